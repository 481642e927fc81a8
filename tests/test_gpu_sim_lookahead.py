"""GPU: the simulator's what-if (mansy_sim_lookahead / mansy_sim_peek_ahead through BatchedSimulator.lookahead / peek(ahead) and
Simulator.lookahead).  A virtual step must return the bits the committed step returns (mansy_sim_download on a cloned state buffer), the
sessions must not move, the recorded sessions of the imported reference (tests/golden/sim_reference.npz) must come out of a look-ahead
as they come out of committed steps, and the best candidate must be the MPC expert's when the candidates are the expert's plans."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _jin2022_tree as jt

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
S = np.load(os.path.join(GOLDEN, 'sim_reference.npz'))
Z = np.load(os.path.join(GOLDEN, 'env_reference.npz'))
FIELDS = ('size', 'quality', 'video_len', 'vp_gt', 'vp_pred', 'vp_acc', 'vp_start', 'vp_end', 'trace_bw', 'trace_len', 'samples')
QOE_W = ((7, 1, 1), (1, 7, 1), (1, 1, 7), (3, 3, 3))


@pytest.fixture(scope='module')
def M():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a ROCm device (no CPU fallback exists)')
    from mansy_immersivevideostreaming_amd.bitrate_selection import simulators
    return simulators


def u32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def synthetic():
    """The tables test_gpu_sim.py::test_against_the_environment_kernel runs on: every session lasts 51 chunks (6..56)."""
    from mansy_immersivevideostreaming_amd.bitrate_selection.envs.mansy_env import EnvTables
    return EnvTables.synthetic('cuda', n_video=5, n_user=4, n_trace=6, n_chunk=60, seed=3, n_sample=37, train_identifier_reward=False)


@pytest.fixture(scope='module')
def ragged():
    """The same tables with the viewport traces cut to four lengths (sessions of 48..51 chunks), so that near the end some sessions
    have fewer chunks left than the horizon while others have more."""
    from mansy_immersivevideostreaming_amd.bitrate_selection.envs.mansy_env import EnvTables
    arrays = dict(synthetic().host)
    arrays['vp_end'] = (arrays['vp_end'] - np.arange(len(arrays['vp_end'])) % 4).astype(np.int32)
    return EnvTables({k: arrays[k] for k in FIELDS}, QOE_W, 'cuda', train_identifier_reward=False)


def golden_tables(tag):
    from mansy_immersivevideostreaming_amd.bitrate_selection.envs.mansy_env import EnvTables
    return EnvTables({k: Z[f'{tag}/{k}'] for k in FIELDS}, Z[f'{tag}/qoe_w'], 'cuda')


def reference(tag, ep):
    return {k: S[f'{tag}/ep{ep}/{k}'] for k in ('ver', 'scalars', 'over', 'qoe', 'ulp_steps')}


def end_chunks(T, sim):
    """end_chunk of the session every record of `sim` holds now (host tables; reset() has advanced the worker mirror by one stride)."""
    h = T.host
    smp = h['samples'][(sim._worker - sim.worker_num) % T.n_sample]
    return np.minimum(h['vp_end'][smp[:, 1]], h['video_len'][smp[:, 0]] - 1)


def commit(M, sim, plans_k):
    """The H steps of one candidate ([n,H,64]) COMMITTED on a clone of sim's state: qoe_parts [n,H,4], scalars [n,H,4], over [n,H]."""
    twin = M.BatchedSimulator(sim.tables, sim.n)
    twin.state.copy_(sim.state)
    qp, sc, ov = [], [], []
    for t in range(plans_k.shape[1]):
        out = twin.simulate_download(plans_k[:, t].contiguous())
        qp.append(out.qoe_parts.cpu().numpy().copy()); sc.append(out.scalars.cpu().numpy().copy()); ov.append(out.over.cpu().numpy().copy())
    return np.stack(qp, 1), np.stack(sc, 1), np.stack(ov, 1)


def f32_running_sum(q, steps):
    """((0 + q_0) + q_1) + .. over t < steps in float32, per row."""
    total = np.zeros(len(q), np.float32)
    for t in range(q.shape[1]):
        total = np.where(t < steps, (total + q[:, t].astype(np.float32)).astype(np.float32), total)
    return total


def check_against_committed(M, sim, plans, closed_at_start):
    n, K, H = plans.shape[:3]
    before = sim.state.clone()
    out = sim.lookahead(plans)
    assert torch.equal(sim.state, before), 'lookahead moved a session'
    qp, sc, total, steps = (x.cpu().numpy() for x in (out.qoe_parts, out.scalars, out.total, out.steps))
    assert qp.shape == (n, K, H, 4) and sc.shape == (n, K, H, 4) and total.shape == (n, K) and steps.shape == (n,)
    assert qp.dtype == np.float32 and sc.dtype == np.float64 and total.dtype == np.float32 and steps.dtype == np.int32
    for name, col in (('qoe', 0), ('qoe1', 1), ('qoe2', 2), ('qoe3', 3)):
        assert torch.equal(getattr(out, name), out.qoe_parts[..., col]), name
    for name, col in (('chunk_size', 0), ('chunk_quality', 1), ('download_time', 2), ('rebuffer_time', 3)):
        assert torch.equal(getattr(out, name), out.scalars[..., col]), name
    for k in range(K):
        cqp, csc, cov = commit(M, sim, plans[:, k])
        # steps before `over` rose: a session that was closed at the start has none, one that stays open over the horizon has H
        want_steps = np.where(closed_at_start, 0, np.where(cov.any(1), cov.argmax(1) + 1, H)).astype(np.int32)
        assert np.array_equal(steps, want_steps), (k, steps, want_steps)
        live = np.arange(H)[None, :] < steps[:, None]
        assert np.array_equal(qp[:, k].view(np.int32)[live], cqp.view(np.int32)[live]), k
        assert np.array_equal(sc[:, k].view(np.int64)[live], csc.view(np.int64)[live]), k
        assert not qp[:, k].view(np.int32)[~live].any() and not sc[:, k].view(np.int64)[~live].any(), k
        assert np.array_equal(u32(total[:, k]), u32(f32_running_sum(cqp[:, :, 0], steps))), k
    assert torch.equal(sim.state, before)
    short = sim.lookahead(plans, per_step=False)
    assert not hasattr(short, 'qoe_parts') and torch.equal(short.total.cpu(), torch.from_numpy(total))
    assert torch.equal(sim.state, before)
    return steps


def test_virtual_steps_equal_committed_steps_bit_for_bit(M, ragged):
    """n = 37 (a tail workgroup), K = 7, H = 5, at four points of the sessions' lives: right after reset(), after 20 committed steps,
    four chunks before the shortest session ends (steps < H for some, H for others; the committed clones run into closed sessions), and
    four steps later (the shortest sessions are closed at the start, the others have one to three chunks left)."""
    n, K, H = 37, 7, 5
    sim = M.BatchedSimulator(ragged, n, seed=9).reset()
    rs = np.random.RandomState(11)
    end = end_chunks(ragged, sim)
    assert sorted(set(end - 5)) == [48, 49, 50, 51]                # session lengths
    done, seen = 0, []
    for advance in (0, 20, 24, 4):
        for _ in range(advance):
            sim.simulate_download(torch.from_numpy(rs.randint(0, 5, size=(n, 64)).astype(np.int32)).cuda())
        done += advance
        plans = torch.from_numpy(rs.randint(0, 5, size=(n, K, H, 64)).astype(np.int32)).cuda()
        left = end - 5 - done
        steps = check_against_committed(M, sim, plans, closed_at_start=left <= 0)
        assert np.array_equal(steps, np.clip(left, 0, H))
        seen.append(set(steps.tolist()))
    assert seen == [{5}, {5}, {4, 5}, {0, 1, 2, 3}]


def test_versions_outside_are_clamped_like_the_committed_step(M, ragged):
    sim = M.BatchedSimulator(ragged, 5, seed=2).reset()
    plans = torch.from_numpy(np.random.RandomState(5).randint(-3, 9, size=(5, 2, 3, 64)).astype(np.int32)).cuda()
    check_against_committed(M, sim, plans, closed_at_start=np.zeros(5, bool))
    a = sim.lookahead(plans).total.clone()
    assert torch.equal(a, sim.lookahead(plans.clamp(0, 4).contiguous()).total)


def check_virtual_step(ref, t, scalars, qoe_parts):
    """What test_gpu_sim.py::check_step asks of a committed step, for the outputs a virtual step has."""
    where = (t, int(ref['ver'][t][0]))
    assert scalars[0] == ref['scalars'][t, 0] and scalars[1] == ref['scalars'][t, 1], (where, scalars, ref['scalars'][t])
    assert abs(scalars[2] - ref['scalars'][t, 2]) <= 1e-9 and abs(scalars[3] - ref['scalars'][t, 3]) <= 1e-9, (where, scalars, ref['scalars'][t])
    assert u32(qoe_parts[1]) == u32(ref['qoe'][t, 1]) and u32(qoe_parts[3]) == u32(ref['qoe'][t, 3]), (where, qoe_parts, ref['qoe'][t])
    assert abs(int(u32(qoe_parts[0]).item()) - int(u32(ref['qoe'][t, 0]).item())) <= int(ref['ulp_steps'][t]), (where, qoe_parts, ref['qoe'][t])


@pytest.mark.parametrize('sessions', [(0, 1, 2, 3, 4), (2,)])
def test_against_the_imported_reference(M, sessions):
    """Candidate 0 of a session is its own recorded versions of steps t0..t0+7 (checked against the recording), candidate 1 another
    session's (checked against the committed steps), from the fresh reset and after the first 20 recorded steps."""
    T = golden_tables('train_id')
    assert [int(Z[f'train_id/ep{i}/sample_id']) for i in range(5)] == [0, 1, 2, 3, 4]
    n, H = len(sessions), 8
    refs = [reference('train_id', i) for i in sessions]
    other = [reference('train_id', (i + 1) % 5) for i in sessions]
    sim = M.BatchedSimulator(T, n, seed=sessions[0], worker_num=T.n_sample).reset()
    for t0 in (0, 20):
        if t0:
            for t in range(t0):
                sim.simulate_download(torch.from_numpy(np.stack([r['ver'][t] for r in refs]).astype(np.int32)).cuda())
        plans = np.stack([np.stack([r['ver'][t0:t0 + H], o['ver'][t0:t0 + H]]) for r, o in zip(refs, other)]).astype(np.int32)
        assert plans.shape == (n, 2, H, 64)
        plans = torch.from_numpy(plans).cuda()
        before = sim.state.clone()
        out = sim.lookahead(plans)
        assert torch.equal(sim.state, before)
        qp, sc, total, steps = (x.cpu().numpy() for x in (out.qoe_parts, out.scalars, out.total, out.steps))
        assert (steps == H).all()
        for i, ref in enumerate(refs):
            assert not ref['over'][t0:t0 + H].any()                 # the recording's over pattern: none of these steps ends the session
            for t in range(H):
                check_virtual_step(ref, t0 + t, sc[i, 0, t], qp[i, 0, t])
        cqp, csc, cov = commit(M, sim, plans[:, 1])
        assert not cov.any()
        assert np.array_equal(qp[:, 1].view(np.int32), cqp.view(np.int32)) and np.array_equal(sc[:, 1].view(np.int64), csc.view(np.int64))
        assert np.array_equal(u32(total), u32(np.stack([f32_running_sum(qp[:, k, :, 0], steps) for k in range(2)], 1)))


def stagger(M, T, n, seed, rs):
    """n sessions on `T`, session i stepped target[i] random chunks: a helper simulator steps all of them and each record is taken over
    after its own number of steps (the records of a state buffer are independent)."""
    sim = M.BatchedSimulator(T, n, seed=seed).reset()
    left = end_chunks(T, sim) - T.startup_download
    target = rs.randint(0, left)                                  # 0 .. length - 1 steps: at least one chunk is left
    target[:3] = left[:3] - 1                                     # some with exactly one chunk left
    target[3] = 0
    helper = M.BatchedSimulator(T, n, seed=seed).reset()
    rec, src = sim.state.view(n, -1), helper.state.view(n, -1)
    for t in range(1, int(target.max()) + 1):
        helper.simulate_download(torch.from_numpy(rs.randint(0, 5, size=(n, 64)).astype(np.int32)).cuda())
        rows = torch.from_numpy(np.nonzero(target == t)[0]).cuda()
        rec[rows] = src[rows]
    assert np.array_equal(sim.peek()['next_chunk'].cpu().numpy(), T.startup_download + 1 + target)
    return sim, left - target


@pytest.mark.parametrize('horizon', [2, 1])
def test_best_candidate_is_the_mpc_experts(M, horizon):
    """The 15^horizon plans of the expert as candidates (plan i = a0 + 15 a1: mansy_allocate_tile_rates of action a_t on the predicted
    map of chunk next_chunk + t): both kernels evaluate the same expressions in the same order on the ground-truth viewport, so the
    winner and its float32 score are the expert's, bit for bit."""
    from mansy_immersivevideostreaming_amd._lib import check, lib, ptr, stream_ptr
    from mansy_immersivevideostreaming_amd.bitrate_selection.envs.expert_env import ExpertCache
    T = synthetic()
    n, K = 64, 15 ** horizon
    h = T.host
    first = T.startup_download + 1
    for vp in sorted(set(h['samples'][:, 1])):                    # no predicted map of a visited chunk is empty
        j0, j1 = first - h['vp_start'][vp], h['vp_end'][vp] - h['vp_start'][vp]
        assert h['vp_pred'][vp, j0:j1 + 1].any(-1).all(), vp
    sim, left = stagger(M, T, n, seed=4, rs=np.random.RandomState(7))
    assert (left == 1).sum() >= 3 and (left >= 2).sum() >= 32
    cache = ExpertCache(T).t
    keys = torch.zeros(n, dtype=torch.int64, device='cuda')
    actions = torch.zeros(n, dtype=torch.int32, device='cuda')
    best_value = torch.zeros(n, dtype=torch.float32, device='cuda')
    best_index = torch.zeros(n, dtype=torch.int64, device='cuda')
    check(lib().mansy_expert_choose_action(ctypes.byref(T.c), ptr(sim.state), n, horizon, ptr(cache['pred_quality']), ptr(cache['pred_var']),
                                           ptr(cache['pred_size']), ptr(keys), ptr(actions), ptr(best_value), ptr(best_index), stream_ptr()),
          'mansy_expert_choose_action')
    rates = (ctypes.c_int * 5)(*T.video_rates)
    per_step = []                                                 # per_step[t][a]: versions [n,64] of action a on chunk next_chunk + t
    for t in range(horizon):
        p = sim.peek(ahead=t)
        if t:
            assert np.array_equal(p['valid'].cpu().numpy(), (left > t).astype(np.uint8))
        pred = p['pred'].float()
        vers = []
        for a in range(15):
            ver = torch.zeros(n, 64, dtype=torch.int32, device='cuda')
            act = torch.full((n,), a, dtype=torch.int32, device='cuda')
            check(lib().mansy_allocate_tile_rates(ptr(pred), ptr(act), n, rates, ptr(ver), stream_ptr()), 'alloc')
            vers.append(ver)
        per_step.append(torch.stack(vers))                        # [15,n,64]
    plans = torch.zeros(n, K, horizon, 64, dtype=torch.int32, device='cuda')
    for i in range(K):
        for t in range(horizon):
            plans[:, i, t] = per_step[t][(i // 15 ** t) % 15]
    out = sim.lookahead(plans, per_step=False)
    assert np.array_equal(out.steps.cpu().numpy(), np.minimum(left, horizon))
    assert np.array_equal(out.best.cpu().numpy().astype(np.int64), best_index.cpu().numpy())
    assert np.array_equal(u32(out.best_total.cpu().numpy()), u32(best_value.cpu().numpy()))
    assert np.array_equal(out.best.cpu().numpy() % 15, actions.cpu().numpy())
    total = out.total.cpu().numpy()
    assert np.array_equal(u32(out.best_total.cpu().numpy()), u32(total[np.arange(n), out.best.cpu().numpy()]))


def test_best_rules_on_a_hand_made_case(M):
    """Two identical plans tie and the lower index wins; an all-zero plan lies strictly below; the winner once more at the end.  A
    session that is closed has no steps, total 0 and best 0."""
    T = synthetic()
    sim = M.BatchedSimulator(T, 1, seed=0)                        # session 0: preference (7, 1, 1), quality dominates
    high = np.full((3, 64), 4, np.int32)
    plans = torch.from_numpy(np.stack([high, high, np.zeros((3, 64), np.int32), high])[None]).cuda()
    out = sim.lookahead(plans)                                    # never reset: closed
    assert out.steps.item() == 0 and out.best.item() == 0 and out.best_total.item() == 0
    assert not out.total.any() and not out.qoe_parts.any() and not out.scalars.any()
    sim.reset()
    out = sim.lookahead(plans)
    total = out.total.cpu().numpy()[0]
    assert out.steps.item() == 3
    assert u32(total[0]) == u32(total[1]) == u32(total[3]) and total[2] < total[0], total
    assert out.best.item() == 0 and u32(out.best_total.cpu().numpy()) == u32(total[0])
    rev = sim.lookahead(plans.flip(1).contiguous())               # [high, zero, high, high]: still the first of the ties
    assert rev.best.item() == 0
    low_first = sim.lookahead(plans[:, [2, 0, 1, 3]].contiguous())
    assert low_first.best.item() == 1 and u32(low_first.best_total.cpu().numpy()) == u32(total[0])
    for _ in range(60):                                           # run the session out: closed again
        sim.simulate_download(plans[:, 0, 0].contiguous())
    assert sim.over.item() == 1
    out = sim.lookahead(plans)
    assert out.steps.item() == 0 and out.best.item() == 0 and out.best_total.item() == 0 and not out.total.any()


def test_peek_ahead(M, ragged):
    from mansy_immersivevideostreaming_amd._lib import check, lib, ptr, stream_ptr
    n = 37
    sim = M.BatchedSimulator(ragged, n, seed=9).reset()
    rs = np.random.RandomState(3)
    for _ in range(46):                                           # the shortest sessions have two chunks left, the longest five
        sim.simulate_download(torch.from_numpy(rs.randint(0, 5, size=(n, 64)).astype(np.int32)).cuda())
    left = end_chunks(ragged, sim) - 5 - 46
    assert sorted(set(left)) == [2, 3, 4, 5]
    p0 = {k: v.clone() for k, v in sim.peek().items()}
    # ahead = 0 through the new entry point == peek()
    d = dict(size=torch.full((n, 5, 64), -1., device='cuda'), quality=torch.full((n, 5, 64), -1., device='cuda'),
             gt=torch.full((n, 64), 7, dtype=torch.uint8, device='cuda'), pred=torch.full((n, 64), 7, dtype=torch.uint8, device='cuda'),
             acc=torch.full((n,), -1., dtype=torch.float64, device='cuda'), valid=torch.full((n,), 7, dtype=torch.uint8, device='cuda'))
    check(lib().mansy_sim_peek_ahead(ctypes.byref(ragged.c), ptr(sim.state), n, 0, ptr(d['size']), ptr(d['quality']), ptr(d['gt']), ptr(d['pred']),
                                     ptr(d['acc']), ptr(d['valid']), stream_ptr()), 'mansy_sim_peek_ahead')
    assert (d['valid'] == 1).all()
    for k in ('size', 'quality', 'gt', 'pred', 'acc'):
        assert torch.equal(d[k], p0[k]), k
    before = sim.state.clone()
    for ahead in (1, 2, 3):
        twin = M.BatchedSimulator(ragged, n)
        twin.state.copy_(sim.state)
        for _ in range(ahead):
            twin.simulate_download(torch.from_numpy(rs.randint(0, 5, size=(n, 64)).astype(np.int32)).cuda())
        want = twin.peek()
        got = sim.peek(ahead=ahead)
        assert torch.equal(sim.state, before)
        valid = got['valid'].cpu().numpy()
        assert np.array_equal(valid, (left > ahead).astype(np.uint8)), ahead        # drops to 0 exactly past end_chunk
        assert 0 < valid.sum() < n or ahead == 1
        for k in ('size', 'quality', 'gt', 'pred', 'acc'):
            assert torch.equal(got[k], want[k]), (ahead, k)
            assert not got[k][torch.from_numpy(valid == 0).cuda()].any(), (ahead, k)
            assert got[k][torch.from_numpy(valid == 1).cuda()].any(), (ahead, k)
            assert got[k].data_ptr() != sim._peek[k].data_ptr()
    for k, v in sim._peek.items():                                # peek()'s own buffers were not written by peek(ahead > 0)
        assert torch.equal(v, p0[k]), k
    closed = M.BatchedSimulator(ragged, 3)                        # never reset: nothing is valid
    got = closed.peek(ahead=1)
    assert not any(v.any() for v in got.values())


@pytest.fixture(scope='module')
def config(tmp_path_factory):
    from mansy_immersivevideostreaming_amd.bitrate_selection.utils.common import get_config_from_yml
    return get_config_from_yml(jt.make_tree(str(tmp_path_factory.mktemp('jin2022_look')), jt.load()))


def test_single_session_lookahead(M, config):
    video, user, trace = (int(x) for x in S['train_id/ep0/ids'])
    sim = M.Simulator(config, 'Jin2022', video, user, '4G', trace, config.startup_download)
    ref = reference('train_id', 0)
    for t in range(3):
        sim.simulate_download(ref['ver'][t])
    plans = np.stack([S[f'train_id/ep{k}/ver'][3:7] for k in range(3)])          # K = 3, H = 4
    chunk, buf = sim.get_next_chunk(), sim.get_buffer_size()
    state = sim._sim.state.clone()
    out = sim.lookahead(plans)
    assert (sim.get_next_chunk(), sim.get_buffer_size()) == (chunk, buf) and torch.equal(sim._sim.state, state)
    assert isinstance(out.steps, int) and out.steps == 4 and isinstance(out.best, int) and 0 <= out.best < 3
    assert out.total.shape == (3,) and out.total.dtype == np.float32 and out.qoe.shape == (3, 4, 4) and out.qoe.dtype == np.float32
    assert out.scalars.shape == (3, 4, 4) and out.scalars.dtype == np.float64
    assert out.best == int(np.argmax(out.total)) and np.array_equal(u32(out.total), u32(f32_running_sum(out.qoe[:, :, 0], 4)))
    for t in range(4):                                            # candidate 0 replays the recording
        sc = out.scalars[0, t]
        assert sc[0] == ref['scalars'][3 + t, 0] and sc[1] == ref['scalars'][3 + t, 1]
        assert abs(sc[2] - ref['scalars'][3 + t, 2]) <= 1e-9 and abs(sc[3] - ref['scalars'][3 + t, 3]) <= 1e-9
    r = sim.simulate_download(plans[out.best][0])
    assert (float(r[2]), r[3], r[4], r[5]) == tuple(out.scalars[out.best, 0]) and sim.get_next_chunk() == chunk + 1
    with pytest.raises(Exception, match='plans'):
        sim.lookahead(plans + 5)
