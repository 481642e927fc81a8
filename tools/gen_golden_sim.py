#!/usr/bin/env python3
"""Golden sessions of the reference Simulator + QoEModel (bitrate_selection/simulators/simulator.py, utils/qoe.py) driven by explicit
per-tile rate versions, produced by importing and running the reference with stubs for gym/munch/prettytable only.  Data only.

The sessions are the ones whose tables tests/golden/env_reference.npz already holds (`<tag>/ep<i>/ids` = video, user, trace): the
five of `train_id`, the three of `valid_w3`, and -- tag `scaled` -- the first two of `train_id` again with trace_scale = (4.0e6, 2.0e5),
for which the scaled throughput arrays of the reference's NetworkTrace are recorded too.  Each session is driven the way MANSYEnv.step
does (mansy_env.py:160-164) for all of its steps; the versions cycle through four patterns: (a) independent uniform 0..4 per tile,
(b) all 64 equal, (c) the allocation of a random action on the predicted viewport, (d) version 4 on ground-truth tiles, 0 elsewhere.
Writes tests/golden/sim_reference.npz."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import refstubs  # noqa: E402
refstubs.install()
REF = '/root/reference/bitrate_selection'
sys.path.insert(0, REF)
os.chdir(REF)          # the reference resolves '../config.yml' relative to its own directory
from utils.common import get_config_from_yml, allocate_tile_rates, action2rates  # noqa: E402
from utils.qoe import QoEModel  # noqa: E402
from simulators.simulator import Simulator  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')
SCALE = (4.0e6, 2.0e5)
F = np.float32


def versions(pattern, rs, config, gt, pred):
    if pattern == 0:
        return rs.randint(0, 5, size=64)
    if pattern == 1:
        return np.full(64, rs.randint(0, 5))
    if pattern == 2:
        rin, rout = action2rates(int(rs.randint(0, 15)))
        ver, _ = allocate_tile_rates(rin, rout, pred, config.video_rates, config.tile_num_width, config.tile_num_height)
        return np.asarray(ver)
    return np.where(gt == 1, 4, 0)


def run_session(config, video, user, trace, weights, rs, trace_scale=None):
    sim = Simulator(config, 'Jin2022', video, user, '4G', trace, config.startup_download, trace_scale=trace_scale)
    w = np.array(weights, dtype=F)
    qm = QoEModel(config, *w)
    rec = {k: [] for k in ('ver', 'tile_size', 'tile_quality', 'viewport', 'scalars', 'over', 'qoe', 'ulp')}
    over, t = False, 0
    while not over:
        gt, pred, _ = sim.get_viewport()
        assert gt.sum() >= 1, 'empty ground-truth viewport'
        ver = versions(t % 4, rs, config, gt, pred).astype(np.int64)
        sizes, quals, chunk_size, chunk_quality, download_time, rebuffer_time, actual_viewport, over = sim.simulate_download(list(ver))
        assert (np.asarray(actual_viewport, dtype=F) == gt).all()
        qoe, qoe1, qoe2, qoe3 = qm.calculate_qoe(actual_viewport=gt, tile_quality=quals, rebuffer_time=rebuffer_time)
        assert qoe2 == rebuffer_time
        assert sizes.astype(np.int32).astype(F).tolist() == sizes.tolist() and float(chunk_size) == float(np.int64(chunk_size))
        again = F(F(w[0] * F(qoe1)) - F(w[1] * F(rebuffer_time))) - F(w[2] * F(qoe3))
        rec['ulp'].append(F(again).view(np.uint32) != F(qoe).view(np.uint32))
        rec['ver'].append(ver.astype(np.int8))
        rec['tile_size'].append(sizes.astype(np.int32))          # whole numbers (asserted above): stored as int32, compared as float32
        rec['tile_quality'].append(quals.astype(F))
        rec['viewport'].append(np.asarray(actual_viewport, dtype=np.uint8))
        rec['scalars'].append(np.array([chunk_size, chunk_quality, download_time, rebuffer_time], np.float64))
        rec['over'].append(bool(over))
        rec['qoe'].append(np.array([F(qoe), F(qoe1), F(qoe2), F(qoe3)], F))
        t += 1
    scaled = np.array([x[1] for x in sim.net_trace.trace], np.float64) if trace_scale is not None else None
    return {k: np.stack(v) for k, v in rec.items()}, scaled


def main():
    config = get_config_from_yml()
    Z = np.load(os.path.join(OUT, 'env_reference.npz'))
    out, n_steps, n_ulp = {}, 0, 0
    rs = np.random.RandomState(21)
    plan = [(tag, tag, i, None) for tag, n in (('train_id', 5), ('valid_w3', 3)) for i in range(n)] + \
           [('scaled', 'train_id', i, SCALE) for i in range(2)]
    scaled_bw = []
    for tag, src, i, scale in plan:
        video, user, trace = (int(x) for x in Z[f'{src}/ep{i}/ids'])
        slot = Z[f'{src}/samples'][int(Z[f'{src}/ep{i}/sample_id'])]
        weights = Z[f'{src}/qoe_w'][slot[3]]
        rec, scaled = run_session(config, video, user, trace, weights, rs, trace_scale=scale)
        assert len(rec['over']) == len(Z[f'{src}/ep{i}/act']) == 51 and rec['over'][-1] and not rec['over'][:-1].any()
        for k, v in rec.items():
            out[f'{tag}/ep{i}/{k if k != "ulp" else "ulp_steps"}'] = v
        out[f'{tag}/ep{i}/ids'] = np.array([video, user, trace], np.int32)
        out[f'{tag}/ep{i}/slot'] = np.asarray(slot, np.int32)               # (video, viewport, trace, qoe) slots in <src>'s tables
        n_steps += len(rec['over'])
        n_ulp += int(rec['ulp'].sum())
        if scaled is not None:
            raw = Z[f'{src}/trace_bw'][slot[2], :Z[f'{src}/trace_len'][slot[2]]]
            assert len(raw) == len(scaled)
            scaled_bw.append(scaled)
    assert n_ulp <= 0.02 * n_steps, (n_ulp, n_steps)
    tmax = max(len(s) for s in scaled_bw)
    bw = np.zeros((len(scaled_bw), tmax), np.float64)
    for j, s in enumerate(scaled_bw):
        bw[j, :len(s)] = s
    out['scaled/trace_bw'] = bw
    out['scaled/trace_len'] = np.array([len(s) for s in scaled_bw], np.int32)
    out['scaled/scale'] = np.array(SCALE, np.float64)          # (up, low)
    path = os.path.join(OUT, 'sim_reference.npz')
    np.savez_compressed(path, **out)
    print('written', path, os.path.getsize(path) // 1024, 'KiB;', n_steps, 'steps,', n_ulp, 'ulp steps')


if __name__ == '__main__':
    main()
