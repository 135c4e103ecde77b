"""CPU tests (no kernel launched) of msmp_batch_assemble_f32's C-ABI: every size the header says is refused is refused by return code
before anything is launched, with a message in msmp_last_error.  The pointers are fake addresses: a call that got as far as a launch
would need a device, and the file runs without one."""
import pytest

from helpers import L        # noqa: F401  (a fixture)

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -2          # include/msmp_pde.h
NAME = b'msmp_batch_assemble_f32'


def call(L, **kw):
    """the entry on fake (never dereferenced) addresses; the defaults are a valid call"""
    d = dict(store=4096, n_samples=5, nt=78, comps=1, nx=100, sample_idx=8192, steps=12288, batch=4, tw=25, t_axis=16384, x_grid=20480,
             var_table=24576, n_vars=3, mode=0, x_out=28672, y_out=32768, pos_out=36864, vars_out=40960, stream=None)
    d.update(kw)
    return L.msmp_batch_assemble_f32(d['store'], d['n_samples'], d['nt'], d['comps'], d['nx'], d['sample_idx'], d['steps'], d['batch'], d['tw'],
                                     d['t_axis'], d['x_grid'], d['var_table'], d['n_vars'], d['mode'], d['x_out'], d['y_out'], d['pos_out'],
                                     d['vars_out'], d['stream'])


def refused(L, code, word, **kw):
    """the call returns `code` and leaves a message of its own (naming the entry and `word`) in msmp_last_error"""
    L.msmp_tune(b'no_such_knob', 1)                    # whatever an earlier refusal left is replaced: the message below is this call's
    assert b'unknown key' in L.msmp_last_error()
    assert call(L, **kw) == code, kw
    msg = L.msmp_last_error()
    assert NAME in msg and word in msg, (kw, msg)


def test_the_library_reports_abi_470(L):
    assert L.msmp_version() == 470


@pytest.mark.parametrize('name', ['store', 'sample_idx', 'steps', 't_axis', 'x_grid', 'x_out', 'y_out', 'pos_out', 'var_table', 'vars_out'])
def test_a_null_pointer_is_an_argument_error(L, name):
    refused(L, ERR_ARG, b'null pointer', **{name: None})


@pytest.mark.parametrize('name', ['store', 'sample_idx', 'steps', 't_axis', 'y_out', 'pos_out'])
def test_mode_1_still_needs_what_it_reads_and_writes(L, name):
    refused(L, ERR_ARG, b'null pointer', mode=1, x_out=None, x_grid=None, var_table=None, vars_out=None, **{name: None})


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


@pytest.mark.parametrize('n_vars', [-1, 4])
def test_n_vars_outside_0_to_3_is_an_argument_error(L, n_vars):
    refused(L, ERR_ARG, b'n_vars=%d outside 0..3' % n_vars, n_vars=n_vars)


@pytest.mark.parametrize('mode', [-1, 2])
def test_a_mode_other_than_0_or_1_is_an_argument_error(L, mode):
    refused(L, ERR_ARG, b'mode=%d' % mode, mode=mode)


@pytest.mark.parametrize('tw', [0, 65, -3])
def test_a_time_window_outside_1_to_64_is_unsupported(L, tw):
    refused(L, ERR_UNSUPPORTED, b'time_window %d outside 1..64' % tw, tw=tw, nt=250)


@pytest.mark.parametrize('nt,tw', [(49, 25), (1, 1), (127, 64)])
def test_fewer_than_two_windows_of_time_steps_is_unsupported(L, nt, tw):
    refused(L, ERR_UNSUPPORTED, b'nt=%d holds no window' % nt, nt=nt, tw=tw)
