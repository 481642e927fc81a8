"""CPU: the host side of the search over per-step budget schedules (mansy_sim_lookahead_schedules, mansy_sim_drive_schedules and the
methods over them): the exported and declared symbols and their prototypes against the header, the macro and the Python constants, the
methods' parameter lists, `schedule_digits` against a plain nested-loop enumeration, and the argument errors that are raised before
any launch -- every limit and null pointer of the two calls by return code and message, F^H overflow included.  No compute call here."""
import ctypes
import inspect
import itertools
import os
import re
import types

import numpy as np
import pytest
import torch

from mansy_immersivevideostreaming_amd import _lib, build_ext
from mansy_immersivevideostreaming_amd._lib import MansyError
from mansy_immersivevideostreaming_amd.bitrate_selection import simulators
from mansy_immersivevideostreaming_amd.bitrate_selection.simulators import BatchedSimulator, Simulator
from mansy_immersivevideostreaming_amd.bitrate_selection.simulators import simulator as simmod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW_HEADER = open(os.path.join(ROOT, 'include', 'mansy_hip.h')).read()
HEADER = re.sub(r'/\*.*?\*/', '', RAW_HEADER, flags=re.S)
NAMES = {
    'mansy_sim_lookahead_schedules': ['T', 'state', 'n', 'levels', 'F', 'H', 'throughput', 'network', 'viewport', 'level_plans', 'level_bytes',
                                      'total', 'steps', 'best', 'best_total', 'stream'],
    'mansy_sim_drive_schedules': ['T', 'state', 'n', 'levels', 'F', 'H', 'D', 'throughput', 'network', 'viewport', 'window', 'history', 'count',
                                  'best', 'best_total', 'versions', 'qoe_parts', 'scalars', 'over', 'auto_reset', 'stream'],
}


def test_symbols_exported_and_declared():
    L = ctypes.CDLL(build_ext.ensure_built())
    for name, args in NAMES.items():
        assert hasattr(L, name), name
        assert name in _lib._PROTOS and len(_lib._PROTOS[name]) == len(args), name
    assert _lib.lib().mansy_abi_version() == 9 == _lib.ABI_VERSION   # new symbols only


@pytest.mark.parametrize('name', sorted(NAMES))
def test_prototypes_match_the_header(name):
    """Argument count, names and pointer-vs-int class of the prototype against the header's declaration."""
    m = re.search(r'^int %s\s*\(([^;{]*?)\)\s*;' % name, HEADER, re.M | re.S)
    assert m
    args = [a.strip() for a in m.group(1).replace('\n', ' ').split(',')]
    proto = _lib._PROTOS[name]
    assert len(args) == len(proto) == len(NAMES[name]), args
    for a, t in zip(args, proto):
        assert (t is ctypes.c_void_p) == ('*' in a), (a, t)
        if '*' not in a:
            assert a.split()[0] == 'int' and t is ctypes.c_int, (a, t)
    assert [a.split()[-1].lstrip('*') for a in args] == NAMES[name]
    assert 'const double* levels' in m.group(1)
    if name == 'mansy_sim_lookahead_schedules':
        assert 'const void* state' in m.group(1) and 'const double* throughput' in m.group(1)      # the records and the estimate are only read
    else:
        assert 'void* state' in m.group(1) and 'const void* state' not in m.group(1)               # the records move
        assert ' double* throughput' in m.group(1) and ' double* history' in m.group(1) and ' int* count' in m.group(1)
        # the drive takes mansy_sim_drive_client's list with levels / F in the place of fractions / K
        client = re.search(r'^int mansy_sim_drive_client\s*\(([^;{]*?)\)\s*;', HEADER, re.M | re.S).group(1)
        swapped = re.sub(r'\s+', ' ', client).replace('fractions', 'levels').replace('int K', 'int F')
        assert re.sub(r'\s+', ' ', m.group(1)) == swapped


def test_macro_and_python_constants():
    m = re.search(r'^#define MANSY_SIM_SCHED_MAX_LEVELS\s+(\d+)\s*$', HEADER, re.M)
    assert m and int(m.group(1)) == simmod.SCHED_MAX_LEVELS == 16
    for macro, value in (('MANSY_SIM_MAX_HORIZON', simmod.MAX_HORIZON), ('MANSY_SIM_MAX_CANDIDATES', simmod.MAX_CANDIDATES),
                         ('MANSY_SIM_DRIVE_MAX_DECISIONS', simmod.DRIVE_MAX_DECISIONS), ('MANSY_SIM_EST_MAX_WINDOW', simmod.EST_MAX_WINDOW)):
        m = re.search(r'^#define %s\s+(\d+)\s*$' % macro, HEADER, re.M)
        assert m and int(m.group(1)) == value, macro
    assert simulators.schedule_digits is simmod.schedule_digits    # exported beside the two classes


def test_methods_and_their_parameter_lists():
    assert list(inspect.signature(simmod.schedule_digits).parameters) == ['F', 'H']
    p = inspect.signature(BatchedSimulator.lookahead_schedules).parameters
    assert list(p) == ['self', 'levels', 'horizon', 'throughput', 'network', 'viewport', 'per_leaf']
    assert (p['network'].default, p['viewport'].default, p['per_leaf'].default) == ('estimate', 'pred', True)
    p = inspect.signature(BatchedSimulator.drive_schedules).parameters
    assert list(p) == ['self', 'levels', 'horizon', 'decisions', 'throughput', 'window', 'viewport', 'network', 'auto_reset', 'per_tile']
    assert (p['window'].default, p['viewport'].default, p['network'].default) == (5, 'pred', 'estimate')
    assert p['auto_reset'].default is False and p['per_tile'].default is True
    p = inspect.signature(Simulator.lookahead_schedules).parameters
    assert list(p) == ['self', 'levels', 'horizon', 'throughput', 'network', 'viewport']
    assert (p['network'].default, p['viewport'].default) == ('estimate', 'pred')
    p = inspect.signature(Simulator.drive_schedules).parameters
    assert list(p) == ['self', 'levels', 'horizon', 'decisions', 'throughput', 'window', 'viewport', 'network']
    assert (p['window'].default, p['viewport'].default, p['network'].default) == (5, 'pred', 'estimate')
    # what existed before
    p = inspect.signature(BatchedSimulator.drive_client).parameters
    assert list(p) == ['self', 'fractions', 'horizon', 'decisions', 'throughput', 'window', 'viewport', 'network', 'auto_reset', 'per_tile']
    assert list(inspect.signature(BatchedSimulator.lookahead_client).parameters) == ['self', 'plans', 'throughput', 'viewport', 'per_step']


@pytest.mark.parametrize('F,H', [(1, 1), (2, 3), (3, 2), (16, 3)])
def test_schedule_digits_against_nested_loops(F, H):
    want = np.array(list(itertools.product(range(F), repeat=H)), np.int64)       # lexicographic, step 0 the most significant digit
    got = simmod.schedule_digits(F, H)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.int64 and tuple(got.shape) == (F ** H, H)
    assert np.array_equal(got.numpy(), want)
    k = np.arange(F ** H)
    for t in range(H):                                             # the header's formula
        assert np.array_equal(want[:, t], (k // F ** (H - 1 - t)) % F)


@pytest.mark.parametrize('F,H', [(0, 1), (17, 1), (2, 0), (2, 9), (16, 4), (16, 8), (9, 4), (2.0, 2), (True, 2), (2, None)])
def test_schedule_digits_refuses(F, H):
    with pytest.raises(MansyError, match='F must|horizon must|schedules'):
        simmod.schedule_digits(F, H)


def _tables():
    T = _lib.EnvTables()
    for f in ('size', 'quality', 'video_len', 'vp_gt', 'vp_pred', 'vp_acc', 'vp_start', 'vp_end', 'trace_bw', 'trace_len', 'samples', 'qoe_w'):
        setattr(T, f, 8)                              # non-null table pointers: nothing is launched below, so nothing reads them
    T.n_sample = T.n_chunk_max = T.n_vpchunk_max = T.trace_len_max = 1
    return T


# F^H beyond MANSY_SIM_MAX_CANDIDATES, up to 16^8 = 2^32 (which wraps to 0 in 32 bits) and 15^8 (which does not fit either)
TOO_MANY = ((16, 4), (16, 8), (15, 8), (8, 5), (5, 6), (3, 8), (9, 4))


def test_lookahead_schedules_refuses_null_and_out_of_range_arguments_with_a_message():
    L = _lib.lib()
    T = _tables()
    Tp, p = ctypes.byref(T), ctypes.c_void_p(8)
    assert L.mansy_sim_lookahead_schedules(None, None, 1, None, 1, 1, None, 0, 0, None, None, None, None, None, None, None) < 0
    assert b'sim_lookahead_schedules' in L.mansy_last_error() and b'tables' in L.mansy_last_error()

    def call(state=p, n=1, levels=p, F=1, H=1, throughput=p, network=1, viewport=1, steps=p):
        return L.mansy_sim_lookahead_schedules(Tp, state, n, levels, F, H, throughput, network, viewport, None, None, None, steps, None, None, None)
    cases = [(dict(state=None), b'state'), (dict(levels=None), b'levels'), (dict(throughput=None), b'throughput'), (dict(steps=None), b'steps'),
             (dict(n=0), b'n must'), (dict(n=-3), b'n must'), (dict(F=0), b'F must'), (dict(F=simmod.SCHED_MAX_LEVELS + 1), b'F must'),
             (dict(H=0), b'H must'), (dict(H=simmod.MAX_HORIZON + 1), b'H must'), (dict(n=2 ** 20, F=8, H=4), b'2^31'),
             (dict(network=-1), b'network'), (dict(network=2), b'network'), (dict(viewport=-1), b'viewport'), (dict(viewport=2), b'viewport')]
    cases += [(dict(F=F, H=H), b'F^H') for F, H in TOO_MANY]
    for kwargs, word in cases:
        assert call(**kwargs) < 0, word
        err = L.mansy_last_error()
        assert word in err and b'sim_lookahead_schedules' in err, (word, err)


def test_drive_schedules_refuses_null_and_out_of_range_arguments_with_a_message():
    L = _lib.lib()
    T = _tables()
    Tp, p = ctypes.byref(T), ctypes.c_void_p(8)
    assert L.mansy_sim_drive_schedules(None, None, 1, None, 1, 1, 1, None, 0, 0, 1, None, None, None, None, None, None, None, None, 0, None) < 0
    assert b'sim_drive_schedules' in L.mansy_last_error() and b'tables' in L.mansy_last_error()

    def call(state=p, n=1, levels=p, F=1, H=1, D=1, throughput=p, network=1, viewport=1, window=5, history=p, count=p, over=p):
        return L.mansy_sim_drive_schedules(Tp, state, n, levels, F, H, D, throughput, network, viewport, window, history, count, None, None, None,
                                           None, None, over, 0, None)
    cases = [(dict(state=None), b'state'), (dict(levels=None), b'levels'), (dict(throughput=None), b'throughput'),
             (dict(history=None), b'history'), (dict(count=None), b'count'), (dict(over=None), b'over'),
             (dict(n=0), b'n must'), (dict(n=-3), b'n must'),
             (dict(F=0), b'F must'), (dict(F=simmod.SCHED_MAX_LEVELS + 1), b'F must'),
             (dict(H=0), b'H must'), (dict(H=simmod.MAX_HORIZON + 1), b'H must'),
             (dict(D=0), b'D must'), (dict(D=simmod.DRIVE_MAX_DECISIONS + 1), b'D must'),
             (dict(n=2 ** 20, F=8, H=4), b'2^31'),
             (dict(network=-1), b'network'), (dict(network=2), b'network'),
             (dict(viewport=-1), b'viewport'), (dict(viewport=2), b'viewport'),
             (dict(window=0), b'window'), (dict(window=simmod.EST_MAX_WINDOW + 1), b'window')]
    cases += [(dict(F=F, H=H), b'F^H') for F, H in TOO_MANY]
    for kwargs, word in cases:
        assert call(**kwargs) < 0, word
        err = L.mansy_last_error()
        assert word in err and b'sim_drive_schedules' in err, (word, err)


def _unbuilt(n=3):
    """A BatchedSimulator without a device: the checks under test run before anything touches one."""
    sim = object.__new__(BatchedSimulator)
    sim.n = n
    sim.state = types.SimpleNamespace(device=torch.device('cuda', 0))
    return sim


def test_batched_lookahead_schedules_refuses_bad_arguments_before_any_launch():
    sim = _unbuilt()
    lv, thr = torch.ones(4, dtype=torch.float64), torch.ones(3, dtype=torch.float64)
    with pytest.raises(MansyError, match='levels.*cuda'):
        sim.lookahead_schedules(np.ones(4), 2, thr)
    with pytest.raises(MansyError, match='levels.*float64'):
        sim.lookahead_schedules(lv.float(), 2, thr)
    with pytest.raises(MansyError, match='throughput.*float64'):
        sim.lookahead_schedules(lv, 2, 2.0e6)
    with pytest.raises(MansyError, match='throughput.*float64'):
        sim.lookahead_schedules(lv, 2, None)
    with pytest.raises(MansyError, match='levels.*shape'):
        sim.lookahead_schedules(torch.ones(2, 2, dtype=torch.float64), 2, thr)
    for shape in ((2,), (3, 1), ()):
        with pytest.raises(MansyError, match='throughput.*shape'):
            sim.lookahead_schedules(lv, 2, torch.ones(shape, dtype=torch.float64))
    for F in (0, simmod.SCHED_MAX_LEVELS + 1):
        with pytest.raises(MansyError, match='budget levels'):
            sim.lookahead_schedules(torch.ones(F, dtype=torch.float64), 2, thr)
    for H in (0, simmod.MAX_HORIZON + 1, 2.0, True, None):
        with pytest.raises(MansyError, match='horizon'):
            sim.lookahead_schedules(lv, H, thr)
    for F, H in ((4, 7), (16, 4), (16, 8), (9, 4)):
        with pytest.raises(MansyError, match='schedules'):
            sim.lookahead_schedules(torch.ones(F, dtype=torch.float64), H, thr)
    big = _unbuilt(2 ** 19)
    with pytest.raises(MansyError, match=r'2\^31'):
        big.lookahead_schedules(lv, 6, torch.ones(2 ** 19, dtype=torch.float64))
    for viewport in ('truth', 1, None, b'pred'):
        with pytest.raises(MansyError, match='viewport'):
            sim.lookahead_schedules(lv, 2, thr, viewport=viewport)
    for network in ('oracle', 1, None):
        with pytest.raises(MansyError, match='network'):
            sim.lookahead_schedules(lv, 2, thr, network=network)
    with pytest.raises(MansyError, match='levels.*cuda'):          # everything else is right: where the tensors live comes last
        sim.lookahead_schedules(lv, 2, thr)


def test_batched_drive_schedules_refuses_bad_arguments_before_any_launch():
    sim = _unbuilt()
    lv, thr = torch.ones(4, dtype=torch.float64), torch.ones(3, dtype=torch.float64)
    with pytest.raises(MansyError, match='levels.*cuda'):
        sim.drive_schedules(np.ones(4), 2, 2, thr)
    with pytest.raises(MansyError, match='throughput.*cuda'):
        sim.drive_schedules(lv, 2, 2, 2.0e6)
    with pytest.raises(MansyError, match='levels.*float64'):
        sim.drive_schedules(lv.float(), 2, 2, thr)
    with pytest.raises(MansyError, match='levels.*shape'):
        sim.drive_schedules(torch.ones(2, 2, dtype=torch.float64), 2, 2, thr)
    with pytest.raises(MansyError, match='throughput.*shape'):
        sim.drive_schedules(lv, 2, 2, torch.ones(2, dtype=torch.float64))
    for F in (0, simmod.SCHED_MAX_LEVELS + 1):
        with pytest.raises(MansyError, match='budget levels'):
            sim.drive_schedules(torch.ones(F, dtype=torch.float64), 2, 2, thr)
    for H in (0, simmod.MAX_HORIZON + 1, 2.0, True, None):
        with pytest.raises(MansyError, match='horizon'):
            sim.drive_schedules(lv, H, 2, thr)
    for F, H in ((4, 7), (16, 4), (16, 8)):
        with pytest.raises(MansyError, match='schedules'):
            sim.drive_schedules(torch.ones(F, dtype=torch.float64), H, 2, thr)
    for D in (0, simmod.DRIVE_MAX_DECISIONS + 1, 2.0, True, None):
        with pytest.raises(MansyError, match='decisions'):
            sim.drive_schedules(lv, 2, D, thr)
    for window in (0, simmod.EST_MAX_WINDOW + 1, 2.0, True, None):
        with pytest.raises(MansyError, match='window'):
            sim.drive_schedules(lv, 2, 2, thr, window=window)
    for viewport in ('truth', 0, None):
        with pytest.raises(MansyError, match='viewport'):
            sim.drive_schedules(lv, 2, 2, thr, viewport=viewport)
    for network in ('oracle', 1, None):
        with pytest.raises(MansyError, match='network'):
            sim.drive_schedules(lv, 2, 2, thr, network=network)
    with pytest.raises(MansyError, match='levels.*cuda'):
        sim.drive_schedules(lv, 2, 2, thr)


@pytest.mark.parametrize('levels,horizon,throughput', [
    (np.ones((2, 2)), 2, 1.0e6), (1.5, 2, 1.0e6), (np.ones(0), 2, 1.0e6), (np.ones(17), 2, 1.0e6), ('levels', 2, 1.0e6), (np.ones(3, bool), 2, 1.0e6),
    (np.ones(3), 2, 'fast'), (np.ones(3), 2, None), (np.ones(3), 2, [1.0, 2.0]), (np.ones(3), 0, 1.0e6), (np.ones(3), 9, 1.0e6), (np.ones(16), 4, 1.0e6),
])
def test_single_session_calls_refuse_bad_arguments(levels, horizon, throughput):
    sim = object.__new__(Simulator)                               # no device: the checks come first
    sim.next_chunk, sim.end_chunk = 6, 40
    with pytest.raises(MansyError, match='levels|throughput|horizon|schedules'):
        sim.drive_schedules(levels, horizon, 2, throughput)
    with pytest.raises(MansyError, match='levels|throughput|horizon|schedules'):
        sim.lookahead_schedules(levels, horizon, throughput)
    with pytest.raises(MansyError, match='viewport'):
        sim.lookahead_schedules(np.ones(3), 2, 1.0e6, viewport='truth')
    with pytest.raises(MansyError, match='network'):
        sim.lookahead_schedules(np.ones(3), 2, 1.0e6, network='oracle')
