"""Functional test of the multi-rank code path on ONE GPU: two ranks share the device and talk over gloo
(MANSY_DIST_BACKEND=gloo, MANSY_SHARE_GPU=1 -- RCCL itself refuses two ranks on one GPU).  Everything the 8-GPU bench does
runs for real -- SyncBN statistics hook, flat-gradient all-reduce, sharded environments, return-normaliser merge, the
barrier / max-over-ranks timing protocol and the rank-0 JSON line -- only the transport differs."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_two_ranks_share_one_gpu_over_gloo():
    env = dict(os.environ, MANSY_DIST_BACKEND='gloo', MANSY_SHARE_GPU='1', HSA_ENABLE_IPC_MODE_LEGACY='0')
    with socket.socket() as s:          # a free rendezvous port on this box
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '2', '--warmup', '1', '--no-cpu-baseline',
           '--batch', '256', '--full']
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, r.stdout[-2000:]            # rank 0 only
    out = json.loads(lines[0])
    assert out['n_gpus'] == 2 and out['config']['parallelism'] == 'dp2' and out['config']['global_batch'] == 512
    assert out['value'] > 0 and out['secondary']['value'] > 0 and out['secondary']['n_gpus'] == 2
    assert out['roofline']['launches_per_step'] > 0
    assert 0 < out['final_loss'] < 10
    # replicas stay bit-identical: averaged gradients, synchronised BatchNorm statistics, merged return normaliser
    assert out['replica_param_spread'] == 0.0 and out['secondary']['replica_param_spread'] == 0.0


@pytest.mark.gpu
def test_plain_bench_gpus_2_starts_two_ranks(tmp_path):
    """`python bench.py --gpus 2` with NO launcher around it (the driver's form for its scaling runs): bench.py itself starts
    the two rank processes; the line must say so -- n_gpus 2, the process group's own world size 2, an all-reduce head count
    of 2 -- and the replicas must end bit-identical.  `--gpus 1` stays a single process with no process group.  The plain form prints the
    headline only; with --full the same launch also carries the preflight, the replica spread and the PPO leg."""
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    env.update(MANSY_DIST_BACKEND='gloo', MANSY_SHARE_GPU='1', HSA_ENABLE_IPC_MODE_LEGACY='0')
    plain = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '2', '--warmup', '1', '--batch', '256']
    r = subprocess.run(plain, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, r.stdout[-2000:]            # rank 0 only, relayed by the spawning parent
    out = json.loads(lines[0])
    assert out['n_gpus'] == 2 and out['config']['global_batch'] == 512 and out['steps'] == 2 and out['ms_per_step'] > 0 and out['full'] is False
    assert {k: out['dist'][k] for k in ('backend', 'world_size', 'ranks_reporting', 'launcher')} == {'backend': 'gloo', 'world_size': 2, 'ranks_reporting': 2, 'launcher': 'self-spawn'}
    assert 'roofline' not in out and 'secondary' not in out and 'preflight' not in out['dist'] and 0 < out['final_loss'] < 10
    cmd = plain + ['--no-cpu-baseline', '--full']
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out['n_gpus'] == 2 and out['config']['global_batch'] == 512 and out['secondary']['n_gpus'] == 2
    assert {k: out['dist'][k] for k in ('backend', 'world_size', 'ranks_reporting', 'launcher')} == {'backend': 'gloo', 'world_size': 2, 'ranks_reporting': 2, 'launcher': 'self-spawn'}
    assert out['dist']['preflight']['world'] == 2 and out['dist']['preflight']['library_allreduce']['ok']
    assert out['replica_param_spread'] == 0.0 and out['secondary']['replica_param_spread'] == 0.0
    assert out['value'] > 0 and out['secondary']['value'] > 0
    # one GPU, two RCCL ranks, no sharing flag: must refuse loudly instead of printing a line
    env.pop('MANSY_SHARE_GPU')
    env.pop('MANSY_DIST_BACKEND')
    import torch
    if torch.cuda.device_count() < 2:
        r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode != 0 and '{"metric"' not in r.stdout and 'need 2 GPUs' in r.stderr
    # the plain (headline-only) form, with the outputs of its last timed step written out
    dump = tmp_path / 'dump'
    one = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1', '--batch', '256',
                          '--no-cpu-baseline', '--dump-outputs', str(dump)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert one.returncode == 0, one.stdout[-2000:] + one.stderr[-4000:]
    o1 = json.loads([l for l in one.stdout.splitlines() if l.startswith('{"metric"')][0])
    assert o1['n_gpus'] == 1 and o1['dist']['world_size'] == 1 and o1['dist']['backend'] is None
    assert o1['steps'] == 2 and o1['ms_per_step'] > 0 and o1['full'] is False and 'roofline' not in o1 and 'secondary' not in o1
    loss, params = np.load(dump / 'loss.npy'), np.load(dump / 'params.npy')
    assert loss.dtype == np.float32 and loss.shape == (1,) and float(loss[0]) == np.float32(o1['final_loss'])
    assert params.dtype == np.float32 and params.size > 1_000_000 and np.isfinite(params).all()
    for k in ('bn_running_mean', 'bn_running_var'):
        assert np.isfinite(np.load(dump / (k + '.npy'))).all()


@pytest.mark.gpu
@pytest.mark.parametrize('overlap', ['0', '1'])
def test_two_rank_train_step_equals_whole_batch(tmp_path, overlap):
    """a data-parallel VP step over 2 ranks x 32 rows (SyncBN statistics over the global mini-batch + averaged
    flat gradient) computes the gradient, loss and BatchNorm running statistics of ONE process on all 64 rows (dropout off,
    MTIO repeat branch: the same function either way).  fp32 tolerance: summation order over the batch differs."""
    import numpy as np
    # overlap = 1: the gradient sync bench.py uses -- the engine hook starts the all-reduce of the decoder-side two thirds of the
    # flat buffer on a side stream / second process group while the encoder backward is still being enqueued
    env = dict(os.environ, MANSY_DIST_BACKEND='gloo', MANSY_SHARE_GPU='1', HSA_ENABLE_IPC_MODE_LEGACY='0', MANSY_OVERLAP=overlap)
    probe = os.path.join(ROOT, 'tools', 'dp_equiv.py')
    one, two = str(tmp_path / 'one.npz'), str(tmp_path / 'two.npz')
    single_env = {k: v for k, v in env.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
    r = subprocess.run([sys.executable, probe, one], cwd=ROOT, env=single_env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', str(port), probe, two]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    a, b = np.load(one), np.load(two)
    assert int(a['world']) == 1 and int(b['world']) == 2
    np.testing.assert_allclose(b['loss'], a['loss'], rtol=2e-6)
    ga, gb = a['grad'].astype(np.float64), b['grad'].astype(np.float64)
    assert np.linalg.norm(ga) > 0
    assert np.linalg.norm(ga - gb) / np.linalg.norm(ga) < 2e-5, np.linalg.norm(ga - gb) / np.linalg.norm(ga)
    assert np.abs(ga - gb).max() < 1e-4 * np.abs(ga).max()
    np.testing.assert_allclose(b['rm'], a['rm'], atol=1e-6, rtol=1e-5)
    np.testing.assert_allclose(b['rv'], a['rv'], atol=1e-6, rtol=1e-5)


@pytest.mark.gpu
def test_rccl_world1_collectives_of_the_dp_step():
    """RCCL itself (backend "nccl", `device_id=` init) executed on the one GPU there is: WORLD_SIZE=1 in a fresh process, the exact
    collectives of the data-parallel step -- fp32 AVG over the 36.8 MB / 1.7 MB / 1.05 MB flat gradients, the fp64 SUM of the
    2 x 512 SyncBN statistics issued from inside the engine's hook, the 3-double all-gather of the return normaliser -- and a
    whole data-parallel VP step through them that reproduces the plain step (tools/rccl_selftest.py)."""
    env = {k: v for k, v in os.environ.items() if k not in ('MANSY_DIST_BACKEND', 'MANSY_SHARE_GPU')}
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    env.update(RANK='0', WORLD_SIZE='1', LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY='0')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'rccl_selftest.py')], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][-1])
    assert out['backend'] == 'nccl' and out['world'] == 1
    assert out['bn_hook_calls'] == 2 and out['bn_hook_shape'] == [2 * 64]          # forward [sum, sumsq] + backward [sum g, sum g xhat]
    assert abs(out['loss_dp'] - out['loss_plain']) <= 2e-6 * abs(out['loss_plain'])
    # after AdamW (lr 1e-3): identical except the parameters whose true gradient is zero (conv bias in front of the BatchNorm, key
    # biases ...): their gradient is rounding noise, and Adam turns noise of either sign into a +-lr step in both runs
    assert out['param_max_diff'] <= 2.1e-3 and out['param_frac_gt_1e-6'] <= 0.02 and out['bn_mean_max_diff'] <= 1e-6
    assert 0 < out['allreduce_avg_1p7MB_us'] < 5000 and 0 < out['allreduce_avg_36MB_us'] < 50000
    # the overlapped sync ran: the engine hook handed over the decoder-side tail (about two thirds of the buffer)
    assert 0.5 * out['flat_elems'] < out['overlap_tail_elems'] < 0.8 * out['flat_elems']


@pytest.mark.gpu
@pytest.mark.parametrize('form', ['copy', 'slot'])
@pytest.mark.parametrize('world', [2, 3])
def test_peer_memory_allreduce_between_processes_sharing_the_gpu(world, form):
    """csrc/xgmi.hip through dist.PeerGradSync: `world` processes on the one GPU map each other's fine-grained exchange buffers
    through hipIpc and run 40 back-to-back one-shot all-reduces of the PPO flat-gradient size; every result must equal the
    rank-ordered float32 average bit for bit on every rank, the partial sums of squares must add up to its squared norm, and no
    wait may time out (tools/xg_selftest.py).  form 'copy': the gradient is copied into the exchange slot by the collective launch
    (mansy_xg_allreduce_avg); 'slot' (round 5): it is produced IN the slot by an earlier launch and the collective only publishes,
    waits and sums (mansy_xg_reduce_avg) -- followed by a copy-form call on the same context (the two forms may alternate)."""
    env = dict(os.environ, MANSY_SHARE_GPU='1', HSA_ENABLE_IPC_MODE_LEGACY='0', XG_SLOT='1' if form == 'slot' else '0')
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(world), '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.join(ROOT, 'tools', 'xg_selftest.py')]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith('{"ranks"')][-1])
    assert len(out['ranks']) == world
    for rec in out['ranks']:
        assert rec['world'] == world and rec['mismatched_elements'] == 0 and rec['plain_call_ok'], rec
        assert rec['sumsq_rel_err'] < 1e-12, rec


@pytest.mark.gpu
def test_bench_two_ranks_with_the_peer_memory_allreduce():
    """The data-parallel PPO update through the one-shot peer-memory all-reduce (MANSY_PEER_SYNC=1): two ranks share the GPU, the
    averaged gradients are bit-identical on both, so the replicas must end bit-identical like they do over the library collective."""
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    env.update(MANSY_DIST_BACKEND='gloo', MANSY_SHARE_GPU='1', HSA_ENABLE_IPC_MODE_LEGACY='0', MANSY_PEER_SYNC='1')
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '2', '--warmup', '1', '--batch', '256', '--no-cpu-baseline', '--full']
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith('{"metric"')][0])
    assert out['n_gpus'] == 2 and out['secondary']['n_gpus'] == 2 and out['secondary']['grad_sync'] == 'peer-memory one-shot (csrc/xgmi.hip)'
    assert out['secondary']['replica_param_spread'] == 0.0 and out['secondary']['value'] > 0
    assert np.isfinite(out['secondary']['final_loss'])


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['auto', 'off', 'one_rank_fails'])
def test_bench_chooses_its_gradient_average_by_probe_and_falls_back_together(case):
    """bench.py's default for the PPO gradient averages: build the peer-memory all-reduce, check it against the library collective on
    the same data, time both, keep the faster correct one -- the decision is taken collectively, so a set-up failure on ONE rank (injected)
    sends EVERY rank to the library collective instead of leaving the others inside an exchange; MANSY_PEER_SYNC=0 skips the probe.
    Two ranks share the GPU over gloo; the replicas end bit-identical either way."""
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT', 'MANSY_PEER_SYNC')}
    env.update(MANSY_DIST_BACKEND='gloo', MANSY_SHARE_GPU='1', HSA_ENABLE_IPC_MODE_LEGACY='0')
    if case == 'off':
        env['MANSY_PEER_SYNC'] = '0'
    if case == 'one_rank_fails':
        env['MANSY_XG_TEST_FAIL_RANK'] = '1'
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '2', '--warmup', '1', '--batch', '256', '--no-cpu-baseline', '--full']
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    sec = json.loads([l for l in r.stdout.splitlines() if l.startswith('{"metric"')][0])['secondary']
    assert sec['n_gpus'] == 2 and sec['replica_param_spread'] == 0.0 and sec['value'] > 0 and np.isfinite(sec['final_loss'])
    gs = sec['grad_sync']
    if case == 'off':
        assert gs == 'torch.distributed all_reduce'
    elif case == 'one_rank_fails':
        assert gs.startswith('torch.distributed all_reduce; probe: peer set-up failed: rank 1: injected set-up failure'), gs
    else:                      # either outcome is legitimate; the line must say which and why (gloo moves the buffer through the host: peer wins here)
        assert 'probe' in gs and (gs.startswith('peer-memory one-shot (csrc/xgmi.hip); probe: peer ') or gs.startswith('torch.distributed all_reduce; probe: ')), gs


@pytest.mark.gpu
def test_bench_eight_ranks_functional_on_the_shared_gpu():
    """The real entry point at the world size the driver's scaling run uses: `bench.py --gpus 8` starts eight rank processes (here they
    share the one GPU over gloo: MANSY_SHARE_GPU=1), tiny VP batch, one cycle.  What must hold at world 8 before a node ever sees it:
    the process group reports eight ranks, the environment partition is 8 x 256 disjoint consecutive blocks of the 2 048 global workers
    (the reference's worker_id / worker_num stride, mansy_env.py:55-56,100-101), the hand-written peer-memory all-reduce imports seven
    peers' buffers (MANSY_PEER_SYNC=1) and leaves the PPO replicas bit-identical, SyncBN + the overlapped gradient all-reduce leave the
    VP replicas identical."""
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    env.update(MANSY_DIST_BACKEND='gloo', MANSY_SHARE_GPU='1', HSA_ENABLE_IPC_MODE_LEGACY='0', MANSY_PEER_SYNC='slot')
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '8', '--steps', '1', '--warmup', '1', '--batch', '64', '--no-cpu-baseline', '--full']
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith('{"metric"')][0])
    assert out['n_gpus'] == 8 and out['dist']['world_size'] == 8 and out['dist']['ranks_reporting'] == 8
    assert out['config']['global_batch'] == 8 * 64 and out['config']['parallelism'] == 'dp8'
    assert out['replica_param_spread'] <= 1e-6 and np.isfinite(out['final_loss'])
    sec = out['secondary']
    assert sec['n_gpus'] == 8 and sec['config']['parallelism'] == 'dp8' and sec['grad_sync'] == 'peer-memory one-shot (csrc/xgmi.hip)'
    assert sec['replica_param_spread'] == 0.0 and sec['value'] > 0 and np.isfinite(sec['final_loss'])
    n = sec['envs_per_gpu']
    assert sec['env_shards'] == [[r_ * n, 8 * n] for r_ in range(8)]
    # round 6: the update half of the cycle is replayed from a captured hipGraph on every rank (peer averages in the exchange-slot form, epoch derived
    # on the device) -- and the replicas above are STILL bit-identical; the run explains itself
    assert sec['update_half'].startswith('hipGraph replay') and sec['grad_sync_report']['chosen'] == 'peer'
    pf = out['dist']['preflight']
    assert pf['world'] == 8 and pf['device_count'] >= 1 and pf['library_allreduce']['ok'] and len(pf['ranks']) == 8
    assert all(v['ok'] for v in pf['peer_ipc'].values()), pf['peer_ipc']
    assert len(pf['can_access_peer']) == pf['device_count'] and isinstance(pf['host_cores'], list)
    assert len(sec['per_rank']['ms_per_cycle']) == 8 and len(sec['per_rank']['host_enqueue_ms_per_cycle']) == 8
    assert 'us_per_average_wire_and_skew' in sec['wire_term'], sec['wire_term']


@pytest.mark.gpu
def test_library_rccl_communicator_wrappers_world1():
    """mansy_comm_* / mansy_allreduce_* (SURVEY 8b's thin wrappers over RCCL communicators, round 5) on a one-rank communicator: RCCL is bound at run
    time, the agreed set-up (RcclComm.try_create) returns a communicator, and the three collectives of the data-parallel hot path -- flat-gradient
    average (fp32, ncclAvg), SyncBN statistics (fp64 sum), return normaliser (fp64 all-gather) -- are the identity over one rank, at the sizes the
    step uses.  (Two ranks on one GPU are refused by RCCL itself; beyond world 1 the wrappers are correct by construction only.)"""
    import torch
    from mansy_immersivevideostreaming_amd import dist as mdist
    dev = torch.device('cuda', torch.cuda.current_device())
    comm, why = mdist.RcclComm.try_create(1, 0, dev)
    assert comm is not None, why
    try:
        for n in (9_212_000, 427_072, 262_144):
            g = torch.randn(n, device=dev)
            ref = g.clone()
            comm(g)
            torch.cuda.synchronize()
            assert torch.equal(g, ref)
        s = torch.randn(2 * 512, dtype=torch.float64, device=dev)
        ref = s.clone()
        comm.sum_f64(s)
        rms = torch.tensor([0.25, 2.0, 4096.0], dtype=torch.float64, device=dev)
        got = comm.allgather_f64(rms)
        torch.cuda.synchronize()
        assert torch.equal(s, ref) and got.shape == (1, 3) and torch.equal(got[0], rms)
    finally:
        comm.close()


@pytest.mark.gpu
def test_bf16_storage_step_in_two_processes_sharing_the_gpu():
    """Round 6 regression: the weight-gradient loop of the bf16-storage mode (csrc/gemm_bf16a.hip, ds_read_b64_tr_b16) had its LDS wait in a separate asm
    statement from the reads, so the compiler could schedule the consumers above it -- invisible in every single-process test, NaN gradients as soon as two
    processes shared the device (longer LDS latencies).  Two ranks share the GPU and run the bf16 VP step data-parallel (gloo) for four steps: every loss, every
    gradient and every parameter stays finite on both (tools/vp_dp2_probe.py)."""
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    env.update(MANSY_DIST_BACKEND='gloo', MANSY_SHARE_GPU='1', HSA_ENABLE_IPC_MODE_LEGACY='0', MODES='bf16x6,bf16', OVERLAP='1')
    with socket.socket() as s_:
        s_.bind(('127.0.0.1', 0))
        port = s_.getsockname()[1]
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1', '--master-port', str(port),
           os.path.join(ROOT, 'tools', 'vp_dp2_probe.py')]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    import re
    recs = re.findall(r'rank (\d) (\S+) step (\d) loss (\S+) grads finite (True|False) params finite (True|False)', r.stdout)      # (two ranks print into one pipe)
    assert len(recs) == 2 * 2 * 4, r.stdout[-2000:]
    assert all(g == 'True' and p_ == 'True' and np.isfinite(float(l)) for _, _, _, l, g, p_ in recs), recs
