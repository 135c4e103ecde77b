"""The decode routes of the solver classes, one case per cell of the route table (decoder.decode_state's docstring): which C-ABI entries of
the decoder stage one forward (and its backward) calls, and how often, for each of the four decoder kinds plus RETURN_DIFF, without and with
grad, under the defaults and with each switch that bears on the stage at 0.  Driven through the public surface only (MODEL_NAMES, model(data),
backward, msmp_tune), so the table is pinned independently of where the dispatch lives.

  condition                              plain kinds ('1d', '2d')                      gated kinds ('gated', 'gated2d')
  no grad                                the inference entry, no switch consulted;     the one gated launch while "wide_dec" and the switches of the
                                         2-D: double_mlp = msmp_linear_swish_f32       fused width-generic path ("wide_msg", ...) are on; 2-D: double_mlp
                                                                                       = one msmp_linear_f32.  Else PyTorch ops: no entry at all
  grad                                   training forward + backward entry while       the same while "dec_bwd" and the fused width-generic path are on
                                         "dec_bwd" is on; else PyTorch ops
  grad, 2-D: double_mlp                  one msmp_mlp_train_fwd_f32 + one msmp_mlp_train_bwd_f32 while "mlp_train" is on, on either decoder route

msmp_linear_f32 and msmp_mlp_train_fwd_f32 also serve the encoder and the wide layers: they are counted inside the model's `_decode` call only,
and the backward of double_mlp is what msmp_mlp_train_bwd_f32 was called beyond once per encoder forward call.
"""
import pytest
import torch

from helpers import mp, restore_wide_switches, synthetic_case, counted, tuned       # noqa: F401  (mp, restore_wide_switches: fixtures)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures('restore_wide_switches')]
TW = 25

# decoder kind (-diff: RETURN_DIFF) -> name in MODEL_NAMES, sub-network that is run, experiment
CLASSES = {'1d': ('MP-PDE', None, 'E2'), '1d-diff': ('MSSMP-PDE', 'diff', 'E2'), '2d': ('MP-PDE2D', None, 'MSWG3'),
           'gated': ('MSGMP-PDE', None, 'E2'), 'gated2d': ('MSGMP-PDE2D', None, 'MSWG3')}
INFER = {'1d': 'msmp_decoder_f32', '2d': 'msmp_decoder2d_f32', 'gated': 'msmp_decoder_gated_f32', 'gated2d': 'msmp_decoder2d_gated_f32'}
TRAIN = {'1d': ('msmp_decoder_train_fwd_f32', 'msmp_decoder_bwd_f32'), '2d': ('msmp_decoder2d_train_fwd_f32', 'msmp_decoder2d_bwd_f32'),
         'gated': ('msmp_decoder_gated_train_fwd_f32', 'msmp_decoder_gated_bwd_f32'),
         'gated2d': ('msmp_decoder2d_gated_train_fwd_f32', 'msmp_decoder2d_gated_bwd_f32')}
SHARED = ('msmp_linear_f32', 'msmp_mlp_train_fwd_f32')          # counted inside _decode only
COUNTED = tuple(INFER.values()) + tuple(n for pair in TRAIN.values() for n in pair) + ('msmp_linear_swish_f32', 'msmp_mlp_train_bwd_f32') + SHARED
SWITCHES = (None, 'dec_bwd', 'wide_dec', 'mlp_train', 'wide_msg')


def expected(kind, grad, off):
    """{entry: calls} of the table above for one forward (+ backward) with the switch `off` at 0 (None: the defaults); entries not called are absent"""
    plain, two_d = not kind.startswith('gated'), kind.endswith('2d')
    calls = {}
    if not grad:
        if plain or off not in ('wide_dec', 'wide_msg'):
            calls[INFER[kind]] = 1
            if two_d:
                calls['msmp_linear_swish_f32' if plain else 'msmp_linear_f32'] = 1
        return calls
    if off != 'dec_bwd' and (plain or off != 'wide_msg'):
        calls.update({name: 1 for name in TRAIN[kind]})
    if two_d and off != 'mlp_train':
        calls.update(msmp_mlp_train_fwd_f32=1, msmp_mlp_train_bwd_f32=1)
    return calls


_CASES = {}


def setup(mp, monkeypatch, label, **kw):
    """(model whose _decode is watched, graph, the call lists, what _decode's calls added to the SHARED entries)"""
    name, sub, exp = CLASSES[label]
    if exp not in _CASES:
        _CASES[exp] = synthetic_case(mp, exp, bsz=2, seed=3)
    case = _CASES[exp]
    torch.manual_seed(7)
    model = mp.solvers.MODEL_NAMES[name](case.pde, time_window=TW, hidden_layer=1, eq_variables={}, **kw).cuda()
    model = getattr(model, sub) if sub else model
    mp.last_status(reset=True)          # range flags that earlier work left would put the model on the exact-fp32 kernels: another route
    calls = {n: counted(mp, monkeypatch, n) for n in COUNTED}
    window = dict.fromkeys(SHARED, 0)
    real = model._decode

    def watched(*args):
        before = {n: len(calls[n]) for n in SHARED}
        out = real(*args)
        for n in SHARED:
            window[n] += len(calls[n]) - before[n]
        return out
    model._decode = watched
    return model, case.graph.to('cuda'), calls, window


def observe(model, graph, grad, calls, window):
    """one forward (with grad: and its backward) -> (out, {decoder-stage entry: calls}, the entries not called left out)"""
    before = {n: len(c) for n, c in calls.items()}
    window.update(dict.fromkeys(SHARED, 0))
    with torch.enable_grad() if grad else torch.no_grad():
        out = model(graph)
        if grad:
            model.zero_grad(set_to_none=True)
            out.sum().backward()
    torch.cuda.synchronize()
    seen = {n: len(c) - before[n] for n, c in calls.items()}
    encoder_mlps = seen['msmp_mlp_train_fwd_f32'] - window['msmp_mlp_train_fwd_f32']
    seen.update(window)
    seen['msmp_mlp_train_bwd_f32'] -= encoder_mlps
    return out, {n: c for n, c in seen.items() if c}


@pytest.mark.parametrize('off', SWITCHES, ids=lambda s: f'{s}=0' if s else 'defaults')
@pytest.mark.parametrize('grad', [False, True], ids=['nograd', 'grad'])
@pytest.mark.parametrize('label', list(CLASSES))
def test_entries_of_the_decoder_stage(mp, monkeypatch, label, grad, off):
    model, graph, calls, window = setup(mp, monkeypatch, label)
    want = expected(label.split('-')[0], grad, off)
    comps = 2 if model.TWO_D else 1
    with tuned(mp.lib(), **({off: 0} if off else {})):
        for call in ('first', 'second'):            # the second: the memo and the caches change no route
            out, seen = observe(model, graph, grad, calls, window)
            assert seen == want, (label, grad, off, call)
            assert out.shape == (graph.x.shape[0], comps * TW) and out.dtype == graph.x.dtype and torch.isfinite(out).all()


def test_refused_sizes_are_asked_once(mp, monkeypatch):
    """MSGMP-PDE2D at width 165, which msmp_decoder2d_gated_f32 refuses by value (it exists at 164): the first no-grad forward makes the
    row GEMM of double_mlp and asks the entry, the second does neither, and both return what the PyTorch ops return (the route of
    "wide_dec" 0).  165 is the one other width at which the class computes anything: its two CNNs map 82 or 83 features to the 25 steps,
    so the halves of every other width fail in the PyTorch ops themselves."""
    model, graph, calls, window = setup(mp, monkeypatch, 'gated2d', hidden_features=165)
    out1, seen1 = observe(model, graph, False, calls, window)
    out2, seen2 = observe(model, graph, False, calls, window)
    assert seen1 == {'msmp_linear_f32': 1, 'msmp_decoder2d_gated_f32': 1} and seen2 == {}
    with tuned(mp.lib(), wide_dec=0):
        ref, seen = observe(model, graph, False, calls, window)
    assert seen == {} and torch.isfinite(ref).all() and ref.shape == (graph.x.shape[0], 2 * TW)
    assert torch.equal(out1, ref) and torch.equal(out2, ref)
