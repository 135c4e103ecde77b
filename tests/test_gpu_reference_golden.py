"""GPU: the LEM, LSTM, GLU, G2, MSSMP and state-saving drop-in classes, and the time windows 20 and 50, against the output of the
REFERENCE's own classes (tests/golden/deep_*.npz of `gen_golden.py recurrent`; helpers.RECURRENT_CASES).  Reads only tests/golden/.
What these fixtures pin and the one thing they cannot (the cell arithmetic of the absent lem_cuda): tests/golden/standins/README.md."""
import numpy as np
import pytest
import torch

from helpers import (EXPERIMENTS, RECURRENT_CASES, recurrent_id, load_recurrent, recurrent_oracle_rollout, graph_of, pde_of, deep_state_dict,
                     assert_parity, err_stats, fp32_floors, tuned)
from helpers import mp       # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

FLOOR_LIMIT = 1e-4      # x max(1, |ref|): where float32 arithmetic itself is farther than this from the reference, the bar of
#                         assert_parity (2 x floor) would be too wide to notice a wrong kernel; such a fixture gets another seed


def make_pde(mp, exp, d):
    pde_name, eqv, unstructured = EXPERIMENTS[exp]
    kw = dict(tmin=float(d['tmin']), tmax=float(d['tmax']), grid_size=[250, 100])
    pde = {'CE': lambda: mp.CE(L=16., **kw), 'WE': lambda: mp.WE(**kw),
           'AD': lambda: mp.AD(L=16., unstructured=unstructured, **kw)}[pde_name]()
    return pde, eqv


def to_data(mp, g):
    return mp.Data(**{k: torch.tensor(v) for k, v in vars(g).items()}).to('cuda')


@pytest.mark.parametrize('case', RECURRENT_CASES, ids=recurrent_id)
def test_recurrent_classes_vs_reference_golden(mp, case):
    """Depth 6 on two graphs with the fixture's seeded parameters (names, order and shapes of the drop-in class's state_dict checked
    against the reference's): the forward on the default kernels and with msmp_tune("split", 0), then every unrolled step through
    the GraphCreator mirror, each against the reference class's output.  Bar: helpers.assert_parity with the float32 evaluations
    of the oracle as the floor (forward: numpy and torch-GPU; unrolled steps: the float32 numpy oracle rolled out from its own
    predictions).  The forward's numpy floor must itself lie within 1e-4 max(1, |ref|), so that the floor cannot hide a failure
    (gen_golden.py RECURRENT_SEEDS).  The floors of the unrolled steps are on record but not limited: a second pass through an
    untrained 1-D gated stack multiplies the first pass's float32 error by 10-30 (up to 1.1e-3 max(1, |ref|) on WE3) whatever the
    seed.  (The split 0 leg found node_update_kernel starting its fp32 accumulators at the bias: the gated 128-wide classes were
    2.7 - 6.6 x the floor, profiles/r20a_reference_golden_recurrent.md.)  The state-saving classes run their own LEMS carry over both steps; after reset_states() the first graph gives the
    first output bit for bit."""
    kind, exp, tw, save = case
    name = recurrent_id(case)
    d = load_recurrent(case)
    pde, eqv = make_pde(mp, exp, d)
    model = getattr(mp, kind)(pde, time_window=tw, eq_variables=eqv, hidden_layer=6, **({} if save is None else {'save_state': save}))
    sd = deep_state_dict(d, {k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict({k: torch.tensor(v) for k, v in sd.items()}, strict=True)
    model.cuda().eval()
    carry = bool(d['save_state'])
    assert carry == hasattr(getattr(model, 'embedding_lem', None), 'reset_states')
    sd64 = {k: v.astype(np.float64) for k, v in sd.items()}
    limit = lambda ref: FLOOR_LIMIT * max(1.0, float(np.abs(ref).max()))

    floors = fp32_floors(kind, sd64, graph_of(d), pde_of(d), tw, eqv, 6)
    floor = err_stats(floors['numpy_f32'], d['out'])[0]
    print(f'{name}: numpy float32 floor {floor:.3e} (limit {limit(d["out"]):.1e})')
    assert floor <= limit(d['out']), floor
    with torch.no_grad():
        with tuned(mp.lib(), split=0):                  # the fp32-MFMA kernels; the shipped setting is back afterwards, also on an error
            out_f32 = model(to_data(mp, graph_of(d)))
        if carry:
            model.embedding_lem.reset_states()
        data = to_data(mp, graph_of(d))
        out = model(data)
    assert out.dtype == data.x.dtype and out.shape == d['out'].shape
    assert_parity('reference_golden_recurrent', name, out.double().cpu().numpy(), d['out'], floors)
    assert_parity('reference_golden_recurrent', name + '/split0', out_f32.double().cpu().numpy(), d['out'], floors)

    n_roll = int(d['n_roll'])
    preds32 = recurrent_oracle_rollout(case, d, sd64, dtype=np.float32)
    gc = mp.GraphCreator(pde, neighbors=3, time_window=tw, device='cuda')
    u = torch.tensor(d['u_super'].astype(np.float64)).cuda()
    pred, step = out, int(d['first_step'])
    for r in range(n_roll):       # experiments/train_helper.py:255-261
        step += tw
        same = [step] * u.shape[0]
        _, labels = gc.create_data(u, same)
        data = gc.create_next_graph(data, pred, labels, same)
        with torch.no_grad():
            pred = model(data)
        ref = d[f'roll{r}']
        floor = err_stats(preds32[r + 1], ref)[0]
        print(f'{name}: unrolled step {r + 1}: numpy float32 floor {floor:.3e} ({floor / max(1.0, float(np.abs(ref).max())):.1e} max(1, |ref|))')
        assert_parity('reference_golden_recurrent', f'{name}/rollout{r + 1}', pred.double().cpu().numpy(), ref, preds32[r + 1])
    if carry:
        assert n_roll == 2
        model.embedding_lem.reset_states()
        with torch.no_grad():
            again = model(to_data(mp, graph_of(d)))
        assert torch.equal(again, out)
