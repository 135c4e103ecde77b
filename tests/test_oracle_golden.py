"""CPU: pin the oracle (oracle/msmp_oracle.py) against the golden vectors generated from the
reference's own code (tests/golden/gen_golden.py).  float64 vs float64, so the bound is 1e-12."""
import numpy as np
import pytest

from oracle import msmp_oracle as O
from helpers import (load, sd_of, graph_of, pde_of, EXPERIMENTS, DEEP_CASES, deep_state_dict, RECURRENT_CASES, recurrent_id, load_recurrent,
                     recurrent_oracle_rollout)

TW = 25
TOL = 1e-12


@pytest.mark.parametrize('exp', ['E2', 'WE3', 'RPU', 'MSWG3'])
def test_graph_tensors_and_edge_index(exp):
    """Rows G1, G2, R1: create_data / create_graph / create_next_graph incl. bit-exact edge_index."""
    d = load(f'graph_{exp}.npz')
    pde_name, eqv, unstructured = EXPERIMENTS[exp]
    pde = pde_of(d)
    u = d['u_super'].astype(np.float64)
    steps = d['steps'].tolist()
    variables = {k[4:]: v for k, v in d.items() if k.startswith('var_')}
    data, labels = O.create_data(u, steps, TW)
    x = np.tile(d['x_grid'][None], (len(u), 1))
    g = O.create_graph(pde_name, pde, 3, TW, data, labels, x, variables, steps, unstructured)
    ref = graph_of(d)
    assert np.array_equal(g.edge_index, ref.edge_index)          # bit-exact, same order
    assert np.array_equal(g.batch, ref.batch)
    assert np.array_equal(g.x, ref.x) and np.array_equal(g.y, ref.y)
    assert np.array_equal(g.pos, ref.pos)
    for k in ('alpha', 'beta', 'gamma', 'bc_left', 'bc_right', 'c', 'a', 'b'):
        if hasattr(ref, k):
            assert np.array_equal(getattr(g, k), getattr(ref, k)), k
    steps2 = d['steps2'].tolist()
    _, labels2 = O.create_data(u, steps2, TW)
    g2 = O.create_next_graph(pde_name, pde, TW, g, d['pred'].astype(np.float64), labels2, steps2)
    ref2 = graph_of(d, 'n_')
    assert np.array_equal(g2.x, ref2.x) and np.array_equal(g2.y, ref2.y) and np.array_equal(g2.pos, ref2.pos)
    assert np.array_equal(g2.edge_index, ref2.edge_index)


def test_edge_degree_histograms():
    """E2 588 edges/graph with in-degrees 94x6, 2x5, 2x4, 2x3; knn graphs in-degree 3."""
    d = load('graph_E2.npz')
    deg = np.bincount(d['g_edge_index'][1][d['g_edge_index'][1] < 100], minlength=100)
    assert deg.sum() == 588 and sorted(np.bincount(deg)[3:].tolist()) == [2, 2, 2, 94]
    for exp in ('WE3', 'RPU'):
        d = load(f'graph_{exp}.npz')
        assert np.all(np.bincount(d['g_edge_index'][1]) == 3)


@pytest.mark.parametrize('cls,lin', [('GNN_Layer', False), ('GNN_LayerLin', True)])
def test_single_layer(cls, lin):
    """Rows L1-L4: message -> mean -> update (pre-norm) and InstanceNorm (post-norm)."""
    d = load(f'layer_{cls}.npz')
    p = O.layer_params({k: v.astype(np.float64) for k, v in sd_of(d).items()}, '')
    f = lambda k: d[k].astype(np.float64)
    r = O.mp_layer(p, f('h'), f('u'), f('pos_x'), f('variables'), d['edge_index'], d['batch'], lin, parts=True)
    assert np.abs(r.pre - d['pre']).max() < TOL
    assert np.abs(r.out - d['out']).max() < 1e-11


@pytest.mark.parametrize('kind', ['MP_PDE_Solver', 'MP_PDE_SolverGated', 'MP_PDE_Solver2D', 'MP_PDE_Solver2DGated'])
def test_solver_forward_and_rollout(kind):
    """Rows S1, L5, R1: full forward of the LEM-free solver classes and the unrolled evaluation loop."""
    d = load(f'solver_{kind}.npz')
    exp = str(d['experiment'])
    pde_name, eqv, unstructured = EXPERIMENTS[exp]
    pde = pde_of(d)
    g = graph_of(d)
    layers = int(d['hidden_layer'])
    sd = sd_of(d)
    out = O.solver_forward(kind, sd, g, pde, TW, eqv, layers)
    assert out.shape == d['out'].shape
    assert np.abs(out - d['out']).max() < 1e-11
    n_roll = int(d['n_roll'])
    if n_roll:
        u = d['u_super'].astype(np.float64)
        preds = O.rollout(kind, sd, g, pde_name, pde, TW, eqv, layers, u, 50, n_roll)
        for r in range(n_roll):
            assert np.abs(preds[r + 1] - d[f'roll{r}']).max() < 1e-10, r


@pytest.mark.parametrize('kind', ['MP_PDE_Solver', 'MP_PDE_SolverGated', 'MP_PDE_Solver2D', 'MP_PDE_Solver2DGated'])
def test_torch_oracle_matches_golden(kind):
    """The torch-CPU edition of the oracle (bench.py's cpu_baseline port) against the same golden vectors."""
    from oracle import msmp_oracle_torch as OT
    d = load(f'solver_{kind}.npz')
    _, eqv, _ = EXPERIMENTS[str(d['experiment'])]
    out = OT.solver_forward(kind, sd_of(d), graph_of(d), pde_of(d), TW, eqv, int(d['hidden_layer']))
    assert np.abs(out - d['out']).max() < 1e-11


def test_torch_oracle_matches_numpy_oracle_lem():
    """The two oracle editions agree on LEM solvers with default-initialised weights at depth 2 (the reference's classes pin both
    editions around the cell in test_recurrent_classes_vs_reference; only the cell arithmetic of the absent lem_cuda is unpinned)."""
    from oracle import msmp_oracle_torch as OT
    import torch
    import msmp_pde_amd as mp
    from helpers import synthetic_case
    torch.manual_seed(1)
    for kind, exp in (('MP_PDE_SolverLEMLinGated', 'E2'), ('MP_PDE_Solver2DLEMLinGated', 'RPU')):
        case = synthetic_case(mp, exp, bsz=2, seed=3, device='cpu')
        model = getattr(mp, kind)(case.pde, time_window=TW, eq_variables=case.eqv, hidden_layer=2)
        sd = {k: v.detach().numpy() for k, v in model.state_dict().items()}
        g = case.graph_np()
        a = O.solver_forward(kind, sd, g, case.pde, TW, case.eqv, 2)
        b = OT.solver_forward(kind, sd, g, case.pde, TW, case.eqv, 2)
        assert np.abs(a - b).max() < 1e-10


def test_float32_noise_floor_recorded():
    """Context for the 1e-5 bar: the same oracle evaluated in float32 differs from float64 by the
    fp32 noise floor; it must itself be well inside the tolerance the HIP path is held to."""
    d = load('solver_MP_PDE_SolverGated.npz')
    pde = pde_of(d)
    g = graph_of(d)
    out32 = O.solver_forward('MP_PDE_SolverGated', sd_of(d), g, pde, TW, {'beta': 0.2}, 2, dtype=np.float32)
    err = np.abs(out32.astype(np.float64) - d['out']).max()
    assert err < 1e-5, err


def test_lem_cell_properties():
    """LEM cell arithmetic (the one part of the LEM path still UNPINNED: lem_cuda's source is absent, and the fixtures of
    `gen_golden.py recurrent` ran our stand-in of the published cell).  Property checks only: with dt=0
    the state stays zero; output is bounded by 1 (convex combination of tanh values)."""
    rng = np.random.default_rng(0)
    nh, ninp, n, t = 16, 4, 7, 5
    w = rng.standard_normal((3 * nh, ninp + nh)); wz = rng.standard_normal((nh, ninp + nh))
    b = rng.standard_normal(3 * nh); bz = rng.standard_normal(nh)
    x = rng.standard_normal((t, n, ninp))
    assert np.all(O.lem_forward(x, w, wz, b, bz, dt=0.0) == 0)
    y = O.lem_forward(x, w, wz, b, bz, dt=1.0)
    assert y.shape == (n, nh) and np.all(np.abs(y) <= 1.0)


@pytest.mark.parametrize('kind,exp', DEEP_CASES)
def test_full_depth_solver_vs_reference(kind, exp):
    """Full depth (hidden_layer = 6, the reference's default): the oracle against the output of the REFERENCE's class with the
    same seeded parameters (tests/golden/deep_*.npz), forward and one unrolled step."""
    d = load(f'deep_{kind}_{exp}.npz')
    pde_name, eqv, unstructured = EXPERIMENTS[exp]
    pde = pde_of(d)
    g = graph_of(d)
    sd = {k: v.astype(np.float64) for k, v in deep_state_dict(d).items()}
    out = O.solver_forward(kind, sd, g, pde, TW, eqv, 6)
    err = np.abs(out - d['out']).max()
    assert err < 1e-9 * max(1.0, np.abs(d['out']).max()), err
    n_roll = int(d['n_roll'])
    if n_roll:
        u = d['u_super'].astype(np.float64)
        preds = O.rollout(kind, sd, g, pde_name, pde, TW, eqv, 6, u, 50, n_roll)
        for r in range(n_roll):
            assert np.abs(preds[r + 1] - d[f'roll{r}']).max() < 1e-8 * max(1.0, np.abs(d[f'roll{r}']).max()), r


@pytest.mark.parametrize('edition', ['numpy', 'torch'])
@pytest.mark.parametrize('case', RECURRENT_CASES, ids=recurrent_id)
def test_recurrent_classes_vs_reference(case, edition):
    """The LEM, LSTM, GLU, G2, MSSMP and state-saving classes, and the time windows 20 and 50, at full depth: both editions of the
    oracle against the output of the REFERENCE's class with the same seeded parameters (`gen_golden.py recurrent`), forward and
    every unrolled step; bars of test_full_depth_solver_vs_reference.  The reference's LEM ran the stand-in of the absent lem_cuda
    (the published cell: that arithmetic alone stays unpinned); input assembly and column order, the LEMcuda parameter layout,
    dt = 1, lemoutput_mlp, gating, the G2 blend, the GLU halves, the MSSMP composition and the LEMS state carry are the
    reference's own code.  State-saving fixtures: the states are carried over both unrolled steps, the carry changes the first
    unrolled step by more than 100 x its bar, and a fresh state dict on the first graph gives `out` again."""
    kind, exp, tw, _ = case
    d = load_recurrent(case)
    sd = {k: v.astype(np.float64) for k, v in deep_state_dict(d).items()}
    preds = recurrent_oracle_rollout(case, d, sd, torch_edition=edition == 'torch')
    n_roll = int(d['n_roll'])
    assert len(preds) == n_roll + 1 and preds[0].shape == d['out'].shape
    rel = lambda a, ref: np.abs(a - ref).max() / max(1.0, np.abs(ref).max())
    err = rel(preds[0], d['out'])
    assert err < 1e-9, err
    for r in range(n_roll):
        assert rel(preds[r + 1], d[f'roll{r}']) < 1e-8, r
    if bool(d['save_state']):
        assert n_roll == 2
        _, eqv, _ = EXPERIMENTS[exp]
        fresh = {}
        again = O.solver_forward(kind, sd, graph_of(d), pde_of(d), tw, eqv, 6, lem_states=fresh)
        assert rel(again, d['out']) < 1e-9 and 'states' in fresh
        d_stateless = dict(d, save_state=np.bool_(False))
        no_carry = recurrent_oracle_rollout(case, d_stateless, sd)
        assert rel(no_carry[1], d['roll0']) > 100 * 1e-8, 'the fixture does not see the state carry'      # a lost carry misses the bar of the unrolled steps by two orders of magnitude at least
