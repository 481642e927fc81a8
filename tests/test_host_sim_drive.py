"""CPU: the host side of the simulator's one-launch planner loop (mansy_sim_drive, BatchedSimulator.drive, Simulator.drive): the
exported and declared symbol, its prototype and limits against the header, the ABI version, and the argument errors that are raised
before any launch.  No compute call here."""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

from mansy_immersivevideostreaming_amd import _lib, build_ext
from mansy_immersivevideostreaming_amd._lib import MansyError
from mansy_immersivevideostreaming_amd.bitrate_selection.simulators import BatchedSimulator, Simulator
from mansy_immersivevideostreaming_amd.bitrate_selection.simulators import simulator as simmod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW_HEADER = open(os.path.join(ROOT, 'include', 'mansy_hip.h')).read()
HEADER = re.sub(r'/\*.*?\*/', '', RAW_HEADER, flags=re.S)
NAMES = ['T', 'state', 'n', 'fractions', 'K', 'H', 'D', 'throughput', 'best', 'best_total', 'versions', 'qoe_parts', 'scalars', 'over',
         'auto_reset', 'stream']


def test_symbol_exported_and_declared():
    L = ctypes.CDLL(build_ext.ensure_built())
    assert hasattr(L, 'mansy_sim_drive')
    assert 'mansy_sim_drive' in _lib._PROTOS and len(_lib._PROTOS['mansy_sim_drive']) == 16
    assert _lib.lib().mansy_abi_version() == 9                     # a new symbol only


def test_prototype_matches_the_header():
    """Argument count, names and pointer-vs-int class of the prototype against the header's declaration."""
    m = re.search(r'^int mansy_sim_drive\s*\(([^;{]*?)\)\s*;', HEADER, re.M | re.S)
    assert m
    args = [a.strip() for a in m.group(1).replace('\n', ' ').split(',')]
    proto = _lib._PROTOS['mansy_sim_drive']
    assert len(args) == len(proto) == 16, args
    for a, t in zip(args, proto):
        assert (t is ctypes.c_void_p) == ('*' in a), (a, t)
        if '*' not in a:
            assert a.split()[0] == 'int' and t is ctypes.c_int, (a, t)
    assert [a.split()[-1].lstrip('*') for a in args] == NAMES
    assert 'const double* fractions' in m.group(1) and ' double* throughput' in m.group(1) and 'unsigned char* over' in m.group(1)
    assert 'void* state' in m.group(1) and 'const void* state' not in m.group(1)       # the records move


def test_limits_match_the_header():
    for macro, value in (('MANSY_SIM_DRIVE_MAX_CANDIDATES', simmod.DRIVE_MAX_CANDIDATES), ('MANSY_SIM_DRIVE_MAX_DECISIONS', simmod.DRIVE_MAX_DECISIONS)):
        m = re.search(r'^#define %s\s+(\d+)\s*$' % macro, HEADER, re.M)
        assert m and int(m.group(1)) == value, macro
    assert (simmod.DRIVE_MAX_CANDIDATES, simmod.DRIVE_MAX_DECISIONS) == (64, 256)
    assert simmod.DRIVE_MAX_CANDIDATES * simmod.MAX_HORIZON * 64 == 32 * 1024           # the plans of a decision as bytes: 32 KB of LDS


def test_methods_exist():
    p = inspect.signature(BatchedSimulator.drive).parameters
    assert list(p) == ['self', 'fractions', 'horizon', 'decisions', 'throughput', 'auto_reset', 'per_tile']
    assert p['auto_reset'].default is False and p['per_tile'].default is True
    assert list(inspect.signature(Simulator.drive).parameters) == ['self', 'fractions', 'horizon', 'decisions', 'throughput']


def test_null_and_out_of_range_arguments_are_refused_with_a_message():
    L = _lib.lib()
    T = _lib.EnvTables()
    for f in ('size', 'quality', 'video_len', 'vp_gt', 'vp_pred', 'vp_acc', 'vp_start', 'vp_end', 'trace_bw', 'trace_len', 'samples', 'qoe_w'):
        setattr(T, f, 8)                              # non-null table pointers: nothing is launched below, so nothing reads them
    T.n_sample = T.n_chunk_max = T.n_vpchunk_max = T.trace_len_max = 1
    Tp, p = ctypes.byref(T), ctypes.c_void_p(8)
    assert L.mansy_sim_drive(None, None, 1, None, 1, 1, 1, None, None, None, None, None, None, None, 0, None) < 0
    assert b'sim_drive' in L.mansy_last_error() and b'tables' in L.mansy_last_error()

    def call(state=p, n=1, fractions=p, K=1, H=1, D=1, throughput=p, over=p):
        return L.mansy_sim_drive(Tp, state, n, fractions, K, H, D, throughput, None, None, None, None, None, over, 0, None)
    for kwargs, word in ((dict(state=None), b'state'), (dict(fractions=None), b'fractions'), (dict(throughput=None), b'throughput'),
                         (dict(over=None), b'over'), (dict(n=0), b'n must'), (dict(n=-3), b'n must'),
                         (dict(K=0), b'K must'), (dict(K=simmod.DRIVE_MAX_CANDIDATES + 1), b'K must'),
                         (dict(H=0), b'H must'), (dict(H=simmod.MAX_HORIZON + 1), b'H must'),
                         (dict(D=0), b'D must'), (dict(D=simmod.DRIVE_MAX_DECISIONS + 1), b'D must')):
        assert call(**kwargs) < 0, word
        err = L.mansy_last_error()
        assert word in err and b'sim_drive' in err, (word, err)


def _unbuilt(n=3):
    """A BatchedSimulator without a device: the checks under test run before anything touches one."""
    sim = object.__new__(BatchedSimulator)
    sim.n = n
    sim.state = types.SimpleNamespace(device=torch.device('cuda', 0))
    return sim


def test_drive_refuses_bad_arguments_before_any_launch():
    """Each message names what is wrong (dtype, then shape, then the limits, then where the tensors live)."""
    sim = _unbuilt()
    fr, thr = torch.ones(4, dtype=torch.float64), torch.ones(3, dtype=torch.float64)
    with pytest.raises(MansyError, match='fractions.*cuda'):
        sim.drive(np.ones(4), 2, 2, thr)                           # not a tensor
    with pytest.raises(MansyError, match='throughput.*cuda'):
        sim.drive(fr, 2, 2, 2.0e6)
    for dtype in (torch.float32, torch.int64):
        with pytest.raises(MansyError, match='fractions.*float64'):
            sim.drive(fr.to(dtype), 2, 2, thr)
        with pytest.raises(MansyError, match='throughput.*float64'):
            sim.drive(fr, 2, 2, thr.to(dtype))
    with pytest.raises(MansyError, match='fractions.*shape'):
        sim.drive(torch.ones(2, 2, dtype=torch.float64), 2, 2, thr)
    for shape in ((2,), (3, 1), ()):
        with pytest.raises(MansyError, match='throughput.*shape'):
            sim.drive(fr, 2, 2, torch.ones(shape, dtype=torch.float64))
    for K in (0, simmod.DRIVE_MAX_CANDIDATES + 1):
        with pytest.raises(MansyError, match='candidates'):
            sim.drive(torch.ones(K, dtype=torch.float64), 2, 2, thr)
    for H in (0, simmod.MAX_HORIZON + 1, 2.0, True, None):
        with pytest.raises(MansyError, match='horizon'):
            sim.drive(fr, H, 2, thr)
    for D in (0, simmod.DRIVE_MAX_DECISIONS + 1, 2.0, True, None):
        with pytest.raises(MansyError, match='decisions'):
            sim.drive(fr, 2, D, thr)
    with pytest.raises(MansyError, match='fractions.*cuda'):       # everything else is right: where the tensors live comes last
        sim.drive(fr, 2, 2, thr)
    with pytest.raises(MansyError, match='fractions.*contiguous'):
        sim.drive(torch.ones(8, dtype=torch.float64)[::2], 2, 2, thr)


@pytest.mark.parametrize('fractions,throughput', [
    (np.ones((2, 2)), 1.0e6), (1.5, 1.0e6), (np.ones(0), 1.0e6), (np.ones(65), 1.0e6), ('fractions', 1.0e6), ([[1.0, 2.0], [3.0]], 1.0e6),
    (np.ones(3, bool), 1.0e6), (np.ones(3), 'fast'), (np.ones(3), None), (np.ones(3), [1.0, 2.0]),
])
def test_single_session_drive_refuses_bad_arguments(fractions, throughput):
    sim = object.__new__(Simulator)                               # no device: the checks come first
    sim.next_chunk, sim.end_chunk = 6, 40
    with pytest.raises(MansyError, match='fractions|throughput'):
        sim.drive(fractions, 2, 2, throughput)
