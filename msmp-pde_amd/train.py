"""Training step of the reference under graph-sharded data parallelism.

Reference (single device): experiments/train_helper.py:91-141 -- pushforward unrolling under no_grad,
then `loss = sqrt(MSELoss(reduction='sum')(pred, graph.y)); loss.backward(); optimizer.step()`.
The loss is sqrt(S) with S = sum over ALL nodes of the batch, which is not a mean of per-shard losses, so
exact data parallelism is:  (1) all-reduce(SUM) the scalar S_k of every rank;  (2) backward S_k scaled by
1/(2 sqrt(S));  (3) all-reduce(SUM) the gradients (one flat ~5 MB buffer: 1.25-1.34 M fp32 parameters),
RCCL over xGMI when the backend is nccl.  Parameters are replicated; every rank must draw the same
`unrolled_graphs` and its own slice of `random_steps`.

Range policy of the optimisation step (`range_policy` of CapturedTrainStep and training_step; optim.AdamW(skip_nonfinite=True)).
The default (fp16-split) matrix path carries node rows with |x| <= 255 and activations with |x| <= 1023; the reference has no such
limit (models_gnn.py:1315-1377) and its loop (experiments/train_helper.py:125-141) simply trains on such data.  Solver.forward
handles the limit for inference (Solver.range_policy); the same semantics for training:
    None     no check: what the step did before the policy existed.
    'auto'   the FIRST call of a capture (the first eager step of a model) is followed by one stream synchronisation and a read of
             the sticky status word (msmp_last_status): if a kernel left the range, the model switches to the exact-fp32 kernels,
             with one MsmpRangeWarning, and THAT step is evaluated again on them (the device had skipped it: see below), so it is
             not dropped.  Later calls read the word at entry without a synchronisation (flags raised by work that has completed
             since): same switch from that call on; the steps in between were skipped on the device, are dropped, and the warning
             counts them.
    'sync'   every call is checked like the first one: no step is ever dropped and the trajectory is the reference's (one stream
             synchronisation per step).
What keeps a step that left the range from reaching the weights is on the device: msmp_status_poison_f32 turns a raised status word
into a NaN in this rank's S_k before the scalar all-reduce (so every rank sees a NaN loss), and the optimizer's finite check +
guarded AdamW (skip_nonfinite) then skips the update on every rank alike.  A NaN or Inf that comes from the data (a NaN in a label)
is skipped the same way; it raises no range status and switches nothing."""
import os
import warnings

import torch
import torch.distributed as dist

from . import _lib
from .reductions import sqerr_sum

_POLICIES = (None, 'auto', 'sync')
_SWITCHED = 1 << 30           # beside the MSMP_STATUS_* bits: the model was switched to the exact-fp32 kernels by somebody else


def _world():
    """Number of ranks; 0 when there is no process group at all (an initialised ONE-rank group still runs its collectives:
    dist.init_from_env(force_group=True) exercises the RCCL path on a single GPU)."""
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 0


def allreduce_gradients(params):
    """SUM-all-reduce the gradients of `params` as one flat buffer (a single collective per step)."""
    params = [p for p in params if p.grad is not None]
    if _world() == 0 or not params:
        return
    flat = torch.cat([p.grad.reshape(-1) for p in params])
    dist.all_reduce(flat, op=dist.ReduceOp.SUM)
    off = 0
    for p in params:
        n = p.grad.numel()
        p.grad.copy_(flat[off:off + n].view_as(p.grad))
        off += n


def _check_policy(policy, optimizer):
    if policy not in _POLICIES:
        raise ValueError(f"range_policy must be None, 'auto' or 'sync', not {policy!r}")
    if policy is not None and not getattr(optimizer, 'skip_nonfinite', False):
        raise ValueError(f'range_policy={policy!r} needs msmp_pde_amd.optim.AdamW(..., capturable=True, skip_nonfinite=True): '
                         'the step that left the range is skipped on the device')


def _range_flags(model, exact, device):
    """What the policy acts on: the sticky status word (unless this step already runs on the exact-fp32 kernels, which have no range
    to leave), plus _SWITCHED if the model was switched while this step was not.  One host read, no synchronisation -- except under
    data parallelism, where the ranks must act together (a new capture's warm-up and a repeated step run collectives): one 4-byte
    all-reduce(MAX) makes the value common."""
    flags = 0 if exact else _lib.last_status()
    if getattr(model, '_range_exact', False) and not exact:
        flags |= _SWITCHED
    if _world() > 1:
        t = torch.tensor([flags], dtype=torch.int32, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        flags = int(t.item())
    return flags


def _new_skips(optimizer):
    """Steps the optimizer's guard skipped since the last call of this function (a host read: synchronises)."""
    total = optimizer.skipped_steps
    new = total - getattr(optimizer, '_msmp_skips_reported', 0)
    optimizer._msmp_skips_reported = total
    return new


def _range_recover(model, optimizer, flags, repeated):
    """The switch of Solver._range_switch for a training step: the model runs on the exact-fp32 kernels from now on, one
    MsmpRangeWarning says how many optimisation steps were dropped, the status word is cleared."""
    skipped = _new_skips(optimizer)                         # synchronises: the work that raised the word has completed
    dropped = max(skipped - (1 if repeated else 0), 0)
    model._range_exact = True
    status = flags & ~_SWITCHED
    what = ('the fp16-split matrix path left its range during training: ' + '; '.join(t for b, t in _lib._STATUS_TEXT.items() if status & b)
            if status else 'the model was switched to the exact-fp32 kernels outside the training step')
    msg = (f'msmp_pde_amd: {type(model).__name__}: {what}.  {dropped} optimisation step(s) were dropped (skipped on the device before the '
           'host saw the flag)' + ('; the step that raised it is evaluated again' if repeated else '') + '.  The model and its training step now '
           'run on the exact-fp32 MFMA kernels (no range limit, about 2x slower).  Rescale the data to keep the fast path.')
    _lib.last_status(reset=True)
    if os.environ.get('MSMP_STRICT_RANGE') == '1':
        raise _lib.MsmpError(msg)
    warnings.warn(msg, _lib.MsmpRangeWarning, stacklevel=4)
    return dropped


def _status_poison(s_local):
    """S_k behind msmp_status_poison_f32: NaN if the sticky status word is raised when the kernel runs, else unchanged.  The float32
    scalar of the library's loss sum is poisoned in place (one one-wave launch); any other dtype (float64 inputs keep PyTorch's sum)
    gets a float32 zero that went through the kernel added to it."""
    if not s_local.is_cuda:
        return s_local
    if s_local.dtype == torch.float32 and s_local.numel() == 1 and s_local.is_contiguous():
        _lib.check(_lib.lib().msmp_status_poison_f32(s_local.data_ptr(), _lib.current_stream()), 'msmp_status_poison_f32')
        return s_local
    flag = torch.empty(1, dtype=torch.float32, device=s_local.device).fill_(0.0)
    _lib.check(_lib.lib().msmp_status_poison_f32(flag.data_ptr(), _lib.current_stream()), 'msmp_status_poison_f32')
    return s_local + flag.to(s_local.dtype).view(s_local.shape)


def _watchable(loss):
    """The float32 scalar the optimizer's finite check reads for `loss` (made where the loss is made: a capture replays it)."""
    return loss if loss.dtype == torch.float32 else loss.detach().float()


def dp_loss_backward(model, graph, range_guard=False):
    """Forward + backward of the reference's loss on this rank's shard; gradients are left all-reduced
    (identical on every rank and equal to the single-device gradient).  Returns the global loss sqrt(S).
    range_guard: this rank's S_k passes through msmp_status_poison_f32 before the scalar all-reduce: if a kernel of ANY forward so
    far left the range of the fp16-split path (the sticky status word is raised), S, the loss RETURNED (NaN) and every rank's
    gradients are not finite, and optim.AdamW(skip_nonfinite=True) skips the update on every rank with no further collective."""
    pred = model(graph)
    s_local = sqerr_sum(pred, graph.y)                      # MSELoss(reduction='sum'), deterministic two-launch kernel on the GPU
    if range_guard:
        s_local = _status_poison(s_local)
    s_total = s_local.detach().clone()
    if _world() > 0:
        dist.all_reduce(s_total, op=dist.ReduceOp.SUM)
    loss = torch.sqrt(s_total)
    (s_local / (2.0 * loss)).backward()
    allreduce_gradients(list(model.parameters()))
    return loss


def _guarded_eager_step(model, graph, optimizer, policy):
    """`dp_loss_backward` + `optimizer.step()` under a range policy (see the module docstring): the rules of CapturedTrainStep without
    a capture."""
    def once():
        optimizer.zero_grad()
        loss = dp_loss_backward(model, graph, range_guard=not getattr(model, '_range_exact', False))
        watched = _watchable(loss)
        optimizer.watch(watched)
        try:
            optimizer.step()
        finally:
            optimizer.unwatch(watched)
        return loss
    dev = graph.x.device
    dp = _world() > 1               # the ranks read the flags together, whatever kernels each of them is on (see _range_flags)
    exact = lambda: bool(getattr(model, '_range_exact', False))
    if dp or not exact():
        flags = _range_flags(model, exact(), dev)
        if flags and not exact():
            _range_recover(model, optimizer, flags, repeated=False)
    probe = (dp or not exact()) and (policy == 'sync' or not getattr(model, '_range_probed_train', False))
    loss = once()
    if probe:
        model._range_probed_train = True
        torch.cuda.current_stream().synchronize()
        flags = _range_flags(model, exact(), dev)
        if flags:
            repeat = optimizer.last_step_skipped            # the same on every rank: gradients and loss are all-reduced
            if not exact():
                _range_recover(model, optimizer, flags, repeated=repeat)
            if repeat:
                loss = once()
    return loss


def training_step(model, creator, u_super, x, variables, random_steps, unrolled_graphs, optimizer, captured=None, range_policy=None):
    """One iteration of training_loop (experiments/train_helper.py:91-141) on this rank's samples.
    captured: a CapturedTrainStep built on a batch of the same structure (same grid, batch size and neighbourhood): forward + loss +
    backward + optimizer update are then ONE hipGraph launch; the pushforward unrolling stays eager (inference kernels).
    range_policy: None, 'auto' or 'sync' (module docstring); handed to `captured` (it replaces the policy the step was built with),
    or applied around the eager `dp_loss_backward` + `optimizer.step()`.  The loss returned for a step the guard skipped is NaN."""
    _begin_step(optimizer, captured, range_policy)
    steps = list(random_steps)
    data, labels = creator.create_data(u_super, steps)
    graph = creator.create_graph(data, labels, x, variables, steps)
    with torch.no_grad():                                   # pushforward trick, :106-112
        for _ in range(unrolled_graphs):
            steps = [s + creator.tw for s in steps]
            _, labels = creator.create_data(u_super, steps)
            pred = model(graph)
            graph = creator.create_next_graph(graph, pred, labels, steps)
    return _finish_step(model, graph, optimizer, captured, range_policy)


def _begin_step(optimizer, captured, range_policy):
    """What an iteration does before its batch is made: the policy check, and zero_grad (eager) or the policy handed to the capture."""
    _check_policy(range_policy, optimizer)
    if captured is None:
        optimizer.zero_grad()
    elif range_policy is not None:
        if captured.range_policy is None:
            raise ValueError('training_step(range_policy=...): `captured` was built without one (its graph holds no status poison); '
                             'build it with CapturedTrainStep(..., range_policy=...)')
        captured.range_policy = range_policy


def _finish_step(model, graph, optimizer, captured, range_policy):
    """Forward, loss, backward and update on the batch `graph` (experiments/train_helper.py:124-145), captured or eager."""
    if captured is not None:
        loss = captured(graph)
    elif range_policy is not None:
        loss = _guarded_eager_step(model, graph, optimizer, range_policy)
    else:
        loss = dp_loss_backward(model, graph)
        optimizer.step()
    lem = getattr(model, 'embedding_lem', None)            # the Save variants start every sample from fresh LEM states (:144-145)
    if hasattr(lem, 'reset_states'):
        lem.reset_states()
    return loss


def dataset_training_step(model, creator, dataset, indices, random_steps, unrolled_graphs, optimizer, captured=None, range_policy=None):
    """`training_step` fed by a data.DeviceDataset: the same iteration (experiments/train_helper.py:91-141) on the samples `indices` of
    the dataset, with dataset.batch / dataset.advance (one launch each) in place of create_data / create_graph / create_next_graph.
    indices / random_steps: lists (range-checked on the host) or device int tensors.
    captured: a CapturedTrainStep built on a batch of this dataset (float32 tensors of the same batch size).  Without unrolling the
    batch is assembled straight into its static tensors (`captured.data`) and replayed: its copies of a tensor onto itself are no-ops.
    With unrolling, as in the eager case, the batch is assembled into a working Data the dataset reuses (create_next_graph rebinds
    graph.x to the prediction, which must not happen to the capture's static tensors) and `captured` copies it in.
    range_policy: as in `training_step`."""
    import copy
    _begin_step(optimizer, captured, range_policy)
    tensors = torch.is_tensor(random_steps)
    steps = random_steps if tensors else list(random_steps)
    if captured is not None and unrolled_graphs == 0:
        graph = dataset.batch(creator, indices, steps, out=captured.data)
    else:
        graph = copy.copy(dataset.working_batch(creator, indices, steps))     # a shallow copy: rebinding graph.x leaves the working Data whole
        with torch.no_grad():                               # pushforward trick, :106-112
            for _ in range(unrolled_graphs):
                steps = steps + creator.tw if tensors else [s + creator.tw for s in steps]
                pred = model(graph)
                graph = dataset.advance(graph, pred, indices, steps)
    return _finish_step(model, graph, optimizer, captured, range_policy)


class CapturedTrainStep:
    """hipGraph of ONE optimisation step on a fixed batch structure: forward, loss, backward and the optimizer update
    (`dp_loss_backward` + `optimizer.step()`, experiments/train_helper.py:125-141) replayed as graph launches.

    The reference's batch of 16 graphs is ~500 kernel launches of a few microseconds each: eager, the iteration is bound by
    the host issuing them.  What makes the capture safe here:
      * every kernel of the step is stream-ordered and takes no host read-back: layers / LEM forward and backward are the library's
        kernels, the bias gradients of the encoder / decoder and the loss sum are its deterministic reductions (reductions.py: no
        library reduction, hence no memset node in the graph), AdamW runs with the step count and learning rate in device memory
        (optim.AdamW(capturable=True));
      * everything the captured launches point at is owned here: static copies of the batch tensors, private layer / backward
        workspaces, the gradients and the packed weight blobs (allocated from the graph's pool during capture), and references to
        the optimizer's moment tensors and device-side step / learning-rate words (checked at every call: see __call__);
      * the weights are re-packed INSIDE the graph (the packed-blob caches are invalidated right before the capture, so every
        replay packs the parameters it is about to use) and the caches are invalidated again after each replay, so an eager
        forward in between (validation) packs the updated parameters.
    The batch STRUCTURE (edge_index, batch vector, node count) is that of `graph` at construction; `__call__(graph)` copies the
    floating-point node tensors (x, y, pos, equation-parameter columns) of another batch of the same structure and replays.

    Building the capture does NOT train: the `warmup` eager iterations it needs (optimizer state, workspaces, structure caches) run
    on the construction batch, and parameters, Adam moments and the step count are put back afterwards, in place -- the
    first call is the first optimisation step, as in the reference's loop.

    Data parallel (world size > 1): the step is THREE graphs with the two collectives of `dp_loss_backward`
    between them, in the same order and arithmetic as the eager path (so the captured trajectory equals the eager DP trajectory):
        graph F: forward + this rank's S_k;   all-reduce(SUM) of the scalar S;
        graph B: loss = sqrt(S), backward of S_k / (2 loss);   ONE flat all-reduce(SUM) of the gradients (RCCL over xGMI);
        graph U: the AdamW update.
    Without a process group (or with a one-rank group) it is ONE graph.

    range_policy: None (no check), 'auto' or 'sync' -- the module docstring; both need optim.AdamW(skip_nonfinite=True).  The capture
    then holds the status poison behind the loss sum (graph F) and the finite check + guarded AdamW as its update (graph U), with the
    captured loss registered through `optimizer.watch`.  Recovering means capturing again with the forward on the exact-fp32
    kernels (`_exact`); building a capture does not train, so neither does that.  `skipped_steps` (the optimizer's count: steps the
    device skipped, a repeated one included) and `dropped_steps` (those never repeated) are kept; the loss returned for a skipped
    step is NaN."""

    def __init__(self, model, optimizer, graph, warmup=3, range_policy=None):
        import copy
        from ._lib import invalidate_packed_weights
        if not all(g.get('capturable') for g in optimizer.param_groups):
            raise RuntimeError('CapturedTrainStep needs msmp_pde_amd.optim.AdamW(..., capturable=True)')
        _check_policy(range_policy, optimizer)
        self.model, self.opt = model, optimizer
        self.range_policy = range_policy
        self.dropped_steps = 0
        self._warmup = warmup
        self._probed = False          # the synchronous first-call check has been done
        self.loss = self._watched = None
        self.data = copy.copy(graph)
        self._float_keys = [k for k in graph.keys() if torch.is_tensor(getattr(graph, k)) and getattr(graph, k).is_floating_point()]
        for k in self._float_keys:
            setattr(self.data, k, getattr(graph, k).clone())
        self._invalidate = invalidate_packed_weights
        self._dp = _world() > 1
        self._capture()

    @property
    def skipped_steps(self):
        """Optimisation steps the guard skipped on the device (optimizer.skipped_steps: a host read, synchronises)."""
        return self.opt.skipped_steps

    def _capture(self):
        """Warm-up and capture on the batch in the static tensors; the forward runs on the kernels the model is on now."""
        from . import autograd as _ag
        from ._lib import invalidate_packed_weights, cached_operands, _Workspace
        model, optimizer, warmup = self.model, self.opt, self._warmup
        guarded = bool(getattr(optimizer, 'skip_nonfinite', False))
        if self._watched is not None:
            optimizer.unwatch(self._watched)              # the previous capture's scalar lives in the pool of the graphs dropped here
            self._watched = None
        self.graph = self._graphs = None
        self._exact = bool(getattr(model, '_range_exact', False))       # Solver.forward puts the forward under _lib.exact_fp32() then
        poison = self.range_policy is not None and not self._exact     # the exact-fp32 kernels have no range to leave
        dev = self.data.x.device
        params = list(model.parameters())
        old_bwd = _ag._bwd_ws.pop(dev, None)              # the backward's grow-only scratch: a private one for the graph
        try:
            with _Workspace.private(dev) as ws:
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                # what the warm-up iterations change: put back afterwards (in place: the captured launches keep pointing at it)
                p0 = [p.detach().clone() for p in params]
                had_state = {id(p): bool(optimizer.state.get(p)) for p in params}
                s0 = {id(p): {k: v.detach().clone() for k, v in optimizer.state[p].items() if torch.is_tensor(v)} for p in params if had_state[id(p)]}
                def _count(g):          # the group's step count before the warm-up: the device word, or (no step taken yet on this optimizer object) the loaded state's
                    if g.get('_msmp_dev'):
                        return int(g['_msmp_dev']['step'].item())
                    ts = [int(optimizer.state[p]['step'].item()) for p in g['params'] if optimizer.state.get(p)]
                    return ts[0] if ts else 0
                d0 = [_count(g) for g in optimizer.param_groups]
                k0 = [int(g['_msmp_dev']['skipped'].item()) if g.get('_msmp_dev') and 'skipped' in g['_msmp_dev'] else 0 for g in optimizer.param_groups]
                with torch.cuda.stream(side):             # eager warm-up: optimizer state, workspaces, structure caches
                    for _ in range(warmup):
                        optimizer.zero_grad(set_to_none=True)
                        dp_loss_backward(model, self.data, range_guard=poison)
                        optimizer.step()
                torch.cuda.current_stream().wait_stream(side)
                torch.cuda.synchronize()
                with torch.no_grad():
                    for p, q in zip(params, p0):
                        p.copy_(q)
                    for p in params:
                        st = optimizer.state.get(p)
                        if not st:
                            continue
                        for k, v in st.items():
                            if torch.is_tensor(v):
                                v.copy_(s0[id(p)][k]) if had_state[id(p)] else v.zero_()
                    for g, d, k in zip(optimizer.param_groups, d0, k0):
                        if g.get('_msmp_dev'):
                            g['_msmp_dev']['step'].fill_(d)
                            if 'skipped' in g['_msmp_dev']:
                                g['_msmp_dev']['skipped'].fill_(k)
                optimizer.zero_grad(set_to_none=True)
                invalidate_packed_weights()               # the pack kernels must be part of the graph
                if not self._dp:
                    self.graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(self.graph):
                        self.loss = dp_loss_backward(model, self.data, range_guard=poison)
                        if guarded:
                            self._watched = _watchable(self.loss)
                            optimizer.watch(self._watched)
                        optimizer.step()
                    self._graphs = [self.graph]
                else:
                    gf, gb, gu = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
                    cap = torch.cuda.Stream()             # ONE capture stream: autograd runs a node's backward on its forward's stream
                    with torch.cuda.graph(gf, stream=cap):
                        pred = model(self.data)
                        self._s_local = sqerr_sum(pred, self.data.y)
                        if poison:
                            self._s_local = _status_poison(self._s_local)
                    self._s_total = self._s_local.detach().clone()
                    with torch.cuda.graph(gb, pool=gf.pool(), stream=cap):
                        self.loss = torch.sqrt(self._s_total)
                        (self._s_local / (2.0 * self.loss)).backward()
                        if guarded:
                            self._watched = _watchable(self.loss)
                    if guarded:
                        optimizer.watch(self._watched)
                    with torch.cuda.graph(gu, pool=gf.pool(), stream=cap):
                        optimizer.step()
                    self._graphs = [gf, gb, gu]
                torch.cuda.synchronize()
            self._ws = ws.buffers()
            self._bwd_ws = _ag._bwd_ws.pop(dev, None)     # pinned: the captured backward points into it
        finally:
            if old_bwd is not None:
                _ag._bwd_ws[dev] = old_bwd
        self._blobs = cached_operands(model)
        self._params = [(p, p.data_ptr()) for p in params]
        # the optimizer-side memory the graph points at: moments, device step count and learning rate (optimizer.load_state_dict
        # replaces the group dicts and the state tensors; a replay would then read and write freed memory)
        self._opt_dev = [g.get('_msmp_dev') for g in optimizer.param_groups]      # by POSITION: load_state_dict installs new group dicts
        self._opt_state = [(p, optimizer.state[p]['exp_avg'], optimizer.state[p]['exp_avg_sq']) for p in params if optimizer.state.get(p)]
        invalidate_packed_weights()                       # the capture-time hook saw no replay: eager users re-pack

    def _check_pointers(self):
        for p, ptr0 in self._params:
            if p.data_ptr() != ptr0:
                raise RuntimeError('CapturedTrainStep: a parameter was re-allocated (model.to(), load_state_dict with assign): capture again')
        groups = self.opt.param_groups
        for i, dev in enumerate(self._opt_dev):
            if i >= len(groups) or groups[i].get('_msmp_dev') is not dev:
                raise RuntimeError('CapturedTrainStep: the optimizer\'s device-side step / learning-rate state was replaced '
                                   '(optimizer.load_state_dict): capture again')
        for p, m, v in self._opt_state:
            st = self.opt.state.get(p)
            if not st or st['exp_avg'] is not m or st['exp_avg_sq'] is not v:
                raise RuntimeError('CapturedTrainStep: the optimizer state tensors were replaced (optimizer.load_state_dict): capture again')

    def _recover(self, flags, repeated):
        if not self._exact:
            self.dropped_steps += _range_recover(self.model, self.opt, flags, repeated)
        self._capture()           # data parallel: by every rank, also one that is on the exact kernels already (the warm-up runs collectives)

    def __call__(self, graph):
        self._check_pointers()
        policy = self.range_policy
        dev = self.data.x.device
        if policy is not None and (self._dp or not self._exact):
            flags = _range_flags(self.model, self._exact, dev)         # raised by replays that have completed since, or a model switched elsewhere
            if flags:
                self._recover(flags, repeated=False)
        for k in self._float_keys:
            getattr(self.data, k).copy_(getattr(graph, k))
        self.opt.sync_lr()                                # a scheduler may have changed param_groups[i]["lr"]
        self._replay()
        if policy is not None and (self._dp or not self._exact) and (policy == 'sync' or not self._probed):
            self._probed = True
            torch.cuda.current_stream().synchronize()
            flags = _range_flags(self.model, self._exact, dev)
            if flags:
                repeat = self.opt.last_step_skipped       # the poison made the device skip this step; the batch is still in the static tensors
                self._recover(flags, repeated=repeat)
                if repeat:
                    self._replay()
        self._invalidate()
        return self.loss.clone()

    def _replay(self):
        if not self._dp:
            self.graph.replay()
        else:
            gf, gb, gu = self._graphs
            gf.replay()
            self._s_total.copy_(self._s_local.detach())
            dist.all_reduce(self._s_total, op=dist.ReduceOp.SUM)
            gb.replay()
            allreduce_gradients([p for p, _ in self._params])
            gu.replay()
