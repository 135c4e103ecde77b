"""CPU tests (no kernel launched) of msmp_eval_window_f32's C-ABI: everything the header says is refused is refused by return code before
anything is launched, with a message in msmp_last_error.  The pointers are fake addresses: a call that got as far as a launch would
need a device, and the file runs without one."""
import pytest

from helpers import L        # noqa: F401  (a fixture)

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -2          # include/msmp_pde.h
NAME = b'msmp_eval_window_f32'


def call(L, **kw):
    """the entry on fake (never dereferenced) addresses; the defaults are a valid call"""
    d = dict(store=4096, n_samples=5, nt=78, comps=1, nx=100, sample_idx=8192, steps=12288, batch=4, tw=25, pred=16384, t_axis=20480,
             err_out=24576, nrm_out=28672, ld=None, pos_out=32768, stream=None)
    d.update(kw)
    if d['ld'] is None:
        d['ld'] = 2 * 64          # room for every comps and tw a test passes: the ld refusal is tested by itself
    return L.msmp_eval_window_f32(d['store'], d['n_samples'], d['nt'], d['comps'], d['nx'], d['sample_idx'], d['steps'], d['batch'], d['tw'],
                                  d['pred'], d['t_axis'], d['err_out'], d['nrm_out'], d['ld'], d['pos_out'], d['stream'])


def refused(L, code, word, **kw):
    """the call returns `code` and leaves a message of its own (naming the entry and `word`) in msmp_last_error"""
    L.msmp_tune(b'no_such_knob', 1)                    # whatever an earlier refusal left is replaced: the message below is this call's
    assert b'unknown key' in L.msmp_last_error()
    assert call(L, **kw) == code, kw
    msg = L.msmp_last_error()
    assert NAME in msg and word in msg, (kw, msg)


def test_the_binding_lists_the_entry(L):
    from msmp_pde_amd import _lib
    assert 'msmp_eval_window_f32' in _lib.SIGNATURES and hasattr(L, 'msmp_eval_window_f32')


@pytest.mark.parametrize('name', ['store', 'sample_idx', 'steps', 'pred', 'err_out', 'nrm_out'])
@pytest.mark.parametrize('with_pos', [True, False])
def test_a_null_pointer_is_an_argument_error(L, name, with_pos):
    extra = {} if with_pos else {'pos_out': None, 't_axis': None}
    refused(L, ERR_ARG, b'null pointer', **{name: None}, **extra)


def test_a_null_time_axis_with_positions_to_write_is_an_argument_error(L):
    refused(L, ERR_ARG, b'pos_out needs t_axis', t_axis=None)


@pytest.mark.parametrize('name', ['batch', 'nx', 'nt', 'n_samples'])
@pytest.mark.parametrize('value', [0, -1])
def test_a_count_below_one_is_an_argument_error(L, name, value):
    refused(L, ERR_ARG, b'bad sizes', **{name: value})


def test_more_samples_than_an_int32_index_reaches_is_an_argument_error(L):
    refused(L, ERR_ARG, b'bad sizes', n_samples=1 << 31)


@pytest.mark.parametrize('batch,nx', [(1 << 16, 1 << 15), (2 ** 31 - 1, 2), (3, 2 ** 30)])
def test_2_to_the_31_nodes_or_more_is_an_argument_error(L, batch, nx):
    refused(L, ERR_ARG, b'2^31 or more', batch=batch, nx=nx)


@pytest.mark.parametrize('comps', [0, 3, -1])
def test_comps_other_than_1_or_2_is_an_argument_error(L, comps):
    refused(L, ERR_ARG, b'comps=%d' % comps, comps=comps)


@pytest.mark.parametrize('comps,tw,ld', [(1, 25, 24), (2, 25, 49), (2, 25, 25), (1, 1, 0), (1, 25, -50), (2, 64, 127)])
def test_a_row_stride_below_the_row_is_an_argument_error(L, comps, tw, ld):
    refused(L, ERR_ARG, b'ld=%d is below' % ld, comps=comps, tw=tw, ld=ld, nt=250)


@pytest.mark.parametrize('tw', [0, 65, -3])
def test_a_time_window_outside_1_to_64_is_unsupported(L, tw):
    refused(L, ERR_UNSUPPORTED, b'time_window %d outside 1..64' % tw, tw=tw, nt=250)


@pytest.mark.parametrize('nt,tw', [(49, 25), (1, 1), (127, 64)])
def test_fewer_than_two_windows_of_time_steps_is_unsupported(L, nt, tw):
    refused(L, ERR_UNSUPPORTED, b'nt=%d holds no window' % nt, nt=nt, tw=tw)
