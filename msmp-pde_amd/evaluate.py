"""Device-resident evaluation: the reference's test loops on a data.DeviceDataset, one kernel launch per forward.

Reference: test() (experiments/train.py:246-293) runs test_timestep_losses and test_unrolled_losses (experiments/train_helper.py:150-296)
after every epoch, and the paper's number comes from compute_L2_norms (:362-471), which unrolls the same trajectories a second time.
Per batch and window those loops slice the labels on the host (create_data), rebuild the graph (create_next_graph: a cat and a slice),
run a float32 MSELoss and move the graph to the device.  Here the labels are never a tensor:

    window_errors      per graph and column, sum_i (pred - y)^2 and sum_i y^2 in float64 against the labels read from the store, and
                       pos[:, 0] of the next window: ONE msmp_eval_window_f32 launch (csrc/eval_kernel.hip);
    rollout            the unrolled trajectory of every sample -> two float64 tables [S, W, comps * tw]; no host read-back;
    unrolled_losses    test_unrolled_losses' return value from the error table;
    l2_norms           compute_L2_norms (through compute_spacetime_L2_norms) from both tables: the same rollout serves both metrics;
    timestep_losses    test_timestep_losses: one forward per (step, batch);
    base_losses        the numerical-baseline half of test_unrolled_losses (:279-289), model-independent, cached on the dataset;
    test               the reference's test() plus the L2 pair and the base mean; the one place that reads values back, once.

CPU tensors and float64 predictions take a PyTorch restatement of the kernel's formulas (the oracle of the tests): a dataset built
with device='cpu' is evaluated by it, with graphs from GraphCreator that carry no edges (the edge builders are device code)."""
import collections
import copy

import torch

from . import _lib
from .data import _tensor

EvalResult = collections.namedtuple('EvalResult', 'unrolled timestep l2_abs l2_rel base')
EvalResult.__doc__ = """What `test` returns, host floats: unrolled = torch.mean(test_unrolled_losses(...)) (the value the reference's test() returns),
timestep = {step: mean loss} (the numbers test_timestep_losses prints), l2_abs / l2_rel = compute_L2_norms(...), base = the mean
'Unrolled forward base losses' (None when the dataset has no u_base)."""


def _index_tensors(dataset, indices, steps):
    """(sample indices, steps) as int64 tensors on the dataset's device, unchecked (the restatement answers a bad one with NaN)."""
    as_long = lambda v: (v if torch.is_tensor(v) else torch.as_tensor(list(v))).to(device=dataset.device, dtype=torch.long).reshape(-1)
    idx, stp = as_long(indices), as_long(steps)
    if idx.shape != stp.shape or not idx.numel():
        raise ValueError(f'window_errors: {idx.numel()} sample indices for {stp.numel()} steps')
    return idx, stp


def _window_errors_torch(dataset, indices, steps, pred, tw, err, nrm, pos):
    """msmp_eval_window_f32 in tensor expressions: the difference is formed in pred's dtype, the sums are float64."""
    idx, stp = _index_tensors(dataset, indices, steps)
    bsz, nx, cols = idx.shape[0], dataset.nx, dataset.comps * tw
    valid = (idx >= 0) & (idx < dataset.n_samples) & (stp >= tw) & (stp <= dataset.nt - tw)
    ic, pc = idx.clamp(0, dataset.n_samples - 1), stp.clamp(tw, dataset.nt - tw)
    win = pc[:, None] + torch.arange(tw, device=dataset.device)[None, :]
    y = dataset.store[ic[:, None], win].permute(0, 3, 2, 1).reshape(bsz * nx, cols)          # [B, tw, comps, nx] -> component-major rows
    d = pred.to(dataset.device) - y.to(pred.dtype)
    nan = torch.full((), float('nan'), dtype=torch.float64, device=dataset.device)
    e = torch.where(valid[:, None], d.double().square().view(bsz, nx, cols).sum(1), nan)
    n = torch.where(valid[:, None], y.double().square().view(bsz, nx, cols).sum(1), nan)
    err = e if err is None else err.copy_(e)
    nrm = n if nrm is None else nrm.copy_(n)
    if pos is not None:
        nxt = pc + tw
        t_next = dataset.t[nxt.clamp(max=dataset.nt - 1)].to(pos.dtype)
        col = pos.view(bsz, nx, 2)[:, :, 0]
        col.copy_(torch.where((nxt <= dataset.nt - tw)[:, None], t_next[:, None], col))
    return err, nrm


def _table(t, name, bsz, cols, device):
    if not (torch.is_tensor(t) and t.dtype == torch.float64 and t.device == device and tuple(t.shape) == (bsz, cols)
            and (cols == 1 or t.stride(1) == 1) and (bsz == 1 or t.stride(0) >= cols)):
        raise ValueError(f'window_errors({name}=): a float64 tensor on {device} of shape {(bsz, cols)} with unit column stride '
                         f'(a row stride above {cols} is fine: the padding is left alone)')
    return t


def window_errors(dataset, indices, steps, pred, tw, err=None, nrm=None, pos=None):
    """(err, nrm), float64 [B, comps * tw]: for graph b, err[b, c tw + k] = sum_i (pred[b nx + i, c tw + k] - y_i)^2 and
    nrm[b, c tw + k] = sum_i y_i^2 with y_i = store[indices[b], steps[b] + k, c, i] -- criterion(pred, graph.y) of the reference's test
    loops before its sum over columns and graphs (experiments/train_helper.py:184, 239), and the two squares of compute_L2_norms
    (:400-401) summed over nodes.  The difference is formed in float32 as `pred - graph.y` is, squares and sums are float64 in the
    fixed order of csrc/eval_kernel.hip: graph b's numbers do not depend on the batch it is in.  ONE msmp_eval_window_f32 launch.
    indices / steps: lists (range-checked on the host, one pinned copy) or device int tensors (unchecked: a bad one gives that graph
    NaN entries).  err / nrm: tables to write into, possibly rows of a larger one (row stride >= comps * tw).  pos: the graph's
    [B nx, 2] float32 positions; where steps[b] + tw still starts a window, pos[:, 0] becomes t[steps[b] + tw], what create_next_graph
    (common/utils.py:454-469) writes for the next step; elsewhere, and in column 1, it keeps its bytes.
    CPU tensors and float64 predictions: the same formulas in PyTorch, the difference formed in pred's dtype."""
    cols, nx = dataset.comps * tw, dataset.nx
    kernel = dataset.device.type == 'cuda' and pred.is_cuda and pred.dtype == torch.float32
    bsz = len(indices)
    if tuple(pred.shape) != (bsz * nx, cols):
        raise ValueError(f'window_errors: pred must be [{bsz * nx}, {cols}] ({bsz} graphs of {nx} nodes, {dataset.comps} x {tw} columns), '
                         f'not {tuple(pred.shape)}')
    if err is not None:
        _table(err, 'err', bsz, cols, dataset.device)
    if nrm is not None:
        _table(nrm, 'nrm', bsz, cols, dataset.device)
    if (err is None) != (nrm is None) or (err is not None and bsz > 1 and err.stride(0) != nrm.stride(0)):
        raise ValueError('window_errors: give err and nrm both or neither, with one row stride')
    if pos is not None and not (tuple(pos.shape) == (bsz * nx, 2) and pos.is_contiguous() and pos.device == dataset.device):
        raise ValueError(f'window_errors(pos=): the contiguous [{bsz * nx}, 2] position tensor of the graph on {dataset.device}')
    if not kernel or (pos is not None and pos.dtype != torch.float32):
        return _window_errors_torch(dataset, indices, steps, pred, tw, err, nrm, pos)
    idx, stp = dataset._indices(tw, indices, steps)
    if err is None:
        err = torch.empty(bsz, cols, dtype=torch.float64, device=dataset.device)
        nrm = torch.empty(bsz, cols, dtype=torch.float64, device=dataset.device)
    ld = err.stride(0) if bsz > 1 else cols
    pred = pred.contiguous()
    _lib.check(_lib.lib().msmp_eval_window_f32(dataset.store.data_ptr(), dataset.n_samples, dataset.nt, dataset.comps, nx, idx.data_ptr(),
                                               stp.data_ptr(), bsz, tw, pred.data_ptr(), dataset.t32.data_ptr(), err.data_ptr(), nrm.data_ptr(),
                                               ld, _lib.ptr(pos), _lib.current_stream()), 'msmp_eval_window_f32')
    return err, nrm


# ---- batches ----------------------------------------------------------------------------------------------------------------------
def _host_batch(dataset, creator, idx, step):
    """create_graph(*create_data(u, steps), x, variables, steps) for a dataset on the CPU; no edges (module docstring)."""
    u = dataset.store[idx]
    data, labels = creator.create_data(u if dataset.comps == 2 else u[:, :, 0], [step] * len(idx))
    variables = {k: _tensor(v).detach().cpu().reshape(-1)[idx.cpu()] for k, v in dataset.variables.items()}
    return creator.create_graph(data, labels, dataset.x[None].repeat(len(idx), 1), variables, [step] * len(idx),
                                edge_index=torch.zeros(2, 0, dtype=torch.long, device=dataset.device))


class _Batches(object):
    """The batches of an evaluation pass in index order, the last one possibly smaller, with everything the loops need already on the
    device: the sample indices once, and a row of equal steps per start step -- no host-to-device copy inside the loops."""

    def __init__(self, dataset, creator, batch_size, indices):
        dataset._check_creator(creator)
        if batch_size < 1:
            raise ValueError(f'batch_size={batch_size}')
        self.ds, self.creator, self.bs = dataset, creator, int(batch_size)
        order = list(range(dataset.n_samples)) if indices is None else [int(i) for i in indices]
        if not order or min(order) < 0 or max(order) >= dataset.n_samples:
            raise IndexError(f'evaluate: sample indices must be a non-empty subset of 0 .. {dataset.n_samples - 1}')
        self.n = len(order)
        self.idx = torch.tensor(order, dtype=torch.int32).to(dataset.device)
        self.spans = [(i0, min(i0 + self.bs, self.n)) for i0 in range(0, self.n, self.bs)]
        self._steps = {}

    def steps(self, step):
        row = self._steps.get(step)
        if row is None:
            row = self._steps[step] = torch.full((min(self.bs, self.n),), step, dtype=torch.int32).to(self.ds.device)
        return row

    def graph(self, i0, i1, step):
        """The batch of the samples i0 .. i1 - 1 at `step`, as a shallow copy: rebinding its x leaves the dataset's working Data whole."""
        idx = self.idx[i0:i1]
        if self.ds.device.type != 'cuda':
            return _host_batch(self.ds, self.creator, idx.long(), step), idx
        return copy.copy(self.ds.working_batch(self.creator, idx, self.steps(step)[:i1 - i0])), idx


def _reset(model):
    lem = getattr(model, 'embedding_lem', None)            # the Save variants carry LEM states: reset where the reference does
    if hasattr(lem, 'reset_states'):
        lem.reset_states()


def _per_batch(per_sample, batch_size):
    """[..., S] -> [..., n_batches]: sums over consecutive groups of `batch_size` samples (the last group may be smaller)."""
    s = per_sample.shape[-1]
    nb = -(-s // batch_size)
    padded = per_sample.new_zeros(per_sample.shape[:-1] + (nb * batch_size,))
    padded[..., :s] = per_sample
    return padded.view(per_sample.shape[:-1] + (nb, batch_size)).sum(-1)


# ---- the loops --------------------------------------------------------------------------------------------------------------------
def rollout(model, creator, dataset, batch_size, nr_gt_steps, indices=None):
    """(err, nrm): two float64 tables [S, W, comps * tw] on the dataset's device, W = len(range(tw nr_gt_steps, nt - tw + 1, tw)):
    row (s, w) is `window_errors` of sample s for the w-th window of its unrolled trajectory -- the loop test_unrolled_losses
    (experiments/train_helper.py:230-277) and compute_L2_norms (:381-454) both run.  Batches of `batch_size` in index order (the last may
    be smaller; indices: a subset, e.g. one rank's shard).  Per batch: dataset.working_batch at tw nr_gt_steps, then per window
    model(graph) under no_grad, one launch that writes straight into slot w of both tables and pos[:, 0] of the next window, and
    graph.x = pred.  The labels are never a tensor and nothing is read back.  The model's range_policy acts as in any forward; for the
    Save variants embedding_lem.reset_states() follows each batch's trajectory (:275-277, :452-454)."""
    tw = creator.tw
    starts = list(range(tw * int(nr_gt_steps), dataset.nt - tw + 1, tw))
    if nr_gt_steps < 1 or not starts:
        raise ValueError(f'rollout: nr_gt_steps={nr_gt_steps} leaves no window of {tw} steps in {dataset.nt} (the first starts at tw * nr_gt_steps >= tw)')
    batches = _Batches(dataset, creator, batch_size, indices)
    cols = dataset.comps * tw
    err = torch.empty(batches.n, len(starts), cols, dtype=torch.float64, device=dataset.device)
    nrm = torch.empty_like(err)
    with torch.no_grad():
        for i0, i1 in batches.spans:
            graph, idx = batches.graph(i0, i1, starts[0])
            for w, step in enumerate(starts):
                pred = model(graph)
                window_errors(dataset, idx, batches.steps(step)[:i1 - i0], pred, tw, err=err[i0:i1, w], nrm=nrm[i0:i1, w], pos=graph.pos)
                graph.x = pred
            _reset(model)
    return err, nrm


def unrolled_losses(err, batch_size, nx_base_resolution):
    """What test_unrolled_losses returns (experiments/train_helper.py:288-296), float64 [n_batches]: per batch the sum over its windows
    of criterion(pred, graph.y) / nx_base_resolution / batch_size -- divided by the `batch_size` argument, not by the size of a smaller
    last batch, as the reference does (:252)."""
    return _per_batch(err.sum((1, 2)), int(batch_size)) / nx_base_resolution / batch_size


def l2_norms(err, nrm, nx, comps=1):
    """(abs, rel) of compute_L2_norms (experiments/train_helper.py:362-471 through compute_spacetime_L2_norms, :298-328) from the tables
    of one `rollout`, 0-d float64 tensors: per sample sqrt(sum / (W tw nx)) of each table (the sum over components, then the mean over
    time and space), the mean over samples, rel = abs / norm.  Everything is summed, so how the reference's unflatten(1, (tw, d)) splits
    the columns does not matter.  comps: 2 for the AD / 2-D experiments (the tables hold comps * tw columns)."""
    cells = err.shape[1] * (err.shape[2] // comps) * nx
    loss = torch.sqrt(err.sum((1, 2)) / cells).mean()
    norm = torch.sqrt(nrm.sum((1, 2)) / cells).mean()
    return loss, loss / norm


def timestep_losses(model, creator, dataset, batch_size, steps=None, indices=None):
    """{step: mean loss} of test_timestep_losses (experiments/train_helper.py:150-203), 0-d float64 device tensors: for every step kept by
    the reference's rule (step == tw or step % tw == 0; default steps tw .. nt - tw as in test(), experiments/train.py:273), per batch
    criterion(pred, graph.y) / batch_size of ONE forward from the true window before `step`, then the mean over batches (the number the
    reference prints).  One dataset.working_batch, one forward and one launch per (step, batch); the Save variants' states are reset
    after each step's pass over the batches, where the reference does it (:198-200)."""
    tw = creator.tw
    steps = range(tw, dataset.nt - tw + 1) if steps is None else steps
    kept = [int(s) for s in steps if not (s != tw and s % tw != 0)]
    bad = [s for s in kept if not tw <= s <= dataset.nt - tw]
    if bad:
        raise ValueError(f'timestep_losses: step {bad[0]} outside {tw} .. {dataset.nt - tw}')
    batches = _Batches(dataset, creator, batch_size, indices)
    err = torch.empty(len(kept), batches.n, dataset.comps * tw, dtype=torch.float64, device=dataset.device)
    nrm = torch.empty_like(err)
    with torch.no_grad():
        for j, step in enumerate(kept):
            for i0, i1 in batches.spans:
                graph, idx = batches.graph(i0, i1, step)
                window_errors(dataset, idx, batches.steps(step)[:i1 - i0], model(graph), tw, err=err[j, i0:i1], nrm=nrm[j, i0:i1])
            _reset(model)
    means = (_per_batch(err.sum(2), batches.bs) / batch_size).mean(1)
    return {step: means[j] for j, step in enumerate(kept)}


def base_losses(dataset, creator, batch_size, nr_gt_steps, nx_base_resolution):
    """The numerical-baseline half of test_unrolled_losses (experiments/train_helper.py:279-289), float64 [n_batches]: per batch the sum
    over the windows of criterion(labels_super, labels_base) / nx_base_resolution / batch_size, from dataset.store and dataset.u_base
    ([S, nt, nx]; AD: the file layout [S, 2, nt, nx]).  Plain PyTorch in float64: it does not depend on the model, so it is computed
    once per argument set and kept on the dataset."""
    if dataset.u_base is None:
        raise ValueError('base_losses: the dataset was built without u_base (DeviceDataset(..., u_base=...) / from_arrays(..., u_base=...)): '
                         'the baseline compares the training resolution with it')
    tw = creator.tw
    key = ('base_losses', tw, int(batch_size), int(nr_gt_steps), float(nx_base_resolution))
    cache = dataset.__dict__.setdefault('_eval_cache', {})
    if key not in cache:
        starts = range(tw * int(nr_gt_steps), dataset.nt - tw + 1, tw)
        if not len(starts):
            raise ValueError(f'base_losses: nr_gt_steps={nr_gt_steps} leaves no window of {tw} steps in {dataset.nt}')
        base = _tensor(dataset.u_base).to(dataset.device, torch.float64)
        base = base.transpose(1, 2) if dataset.comps == 2 else base[:, :, None]
        if tuple(base.shape) != tuple(dataset.store.shape):
            raise ValueError(f'base_losses: u_base gives {tuple(base.shape)} as [S, nt, comps, nx], the store is {tuple(dataset.store.shape)}')
        t0, t1 = starts[0], starts[-1] + tw
        per_sample = (dataset.store[:, t0:t1].double() - base[:, t0:t1]).square().sum((1, 2, 3))
        cache[key] = _per_batch(per_sample, int(batch_size)) / nx_base_resolution / batch_size
    return cache[key]


def test(model, creator, dataset, batch_size, nr_gt_steps, nx_base_resolution, indices=None):
    """The reference's test() (experiments/train.py:246-293) on a DeviceDataset: model.eval(), the timestep losses, ONE rollout, and the
    mean unrolled loss it returns -- plus what the same rollout gives compute_L2_norms, and the base mean, as an EvalResult of host
    numbers.  The only function of this module that reads values back, once, after everything was launched."""
    model.eval()
    per_step = timestep_losses(model, creator, dataset, batch_size, indices=indices)
    err, nrm = rollout(model, creator, dataset, batch_size, nr_gt_steps, indices=indices)
    l2_abs, l2_rel = l2_norms(err, nrm, dataset.nx, comps=dataset.comps)
    values = [unrolled_losses(err, batch_size, nx_base_resolution).mean(), l2_abs, l2_rel]
    if dataset.u_base is not None and indices is None:
        values.append(base_losses(dataset, creator, batch_size, nr_gt_steps, nx_base_resolution).mean())
    keys = list(per_step)
    host = torch.stack(values + [per_step[k] for k in keys]).tolist()
    n = len(values)
    return EvalResult(unrolled=host[0], timestep=dict(zip(keys, host[n:])), l2_abs=host[1], l2_rel=host[2], base=host[3] if n == 4 else None)


test.__test__ = False          # a library function named like the reference's, not a pytest case
