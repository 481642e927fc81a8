#!/usr/bin/env python3
"""What the oracle's knowledge is worth: every visitable catalogue entry of the two real-table fixtures (`train_id` and `valid_w3` of
tests/golden/env_reference.npz) run to its end, without auto_reset, under three planners with the same budget fractions, horizon and
first estimate --
  oracle     `drive`: candidates downloaded on the real trace and scored on the ground-truth viewport, last-sample estimate;
  client_w1  `drive_client(window=1)`: candidates downloaded at the last sample and scored on the predicted viewport;
  client_w5  `drive_client(window=5)`: the same with the harmonic mean of the newest five samples.
Every planner commits on the truth, so the episodes' QoE terms are comparable.  Reported per fixture and planner: episodes, committed
steps, the mean over episodes of the episode's QoE sum and of its per-step QoE, the rebuffered steps and the rebuffer seconds.  No
outcome is required."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mansy_immersivevideostreaming_amd.bitrate_selection.envs.mansy_env import EnvTables  # noqa: E402
from mansy_immersivevideostreaming_amd.bitrate_selection.simulators import BatchedSimulator  # noqa: E402
from mansy_immersivevideostreaming_amd.bitrate_selection.simulators.simulator import DRIVE_MAX_DECISIONS  # noqa: E402

FIELDS = ('size', 'quality', 'video_len', 'vp_gt', 'vp_pred', 'vp_acc', 'vp_start', 'vp_end', 'trace_bw', 'trace_len', 'samples')


def tables(Z, tag):
    arrays = {k: Z[f'{tag}/{k}'] for k in FIELDS}
    arrays['samples'] = arrays['samples'][(arrays['samples'] >= 0).all(1)]      # the entries that hold tables
    return EnvTables(arrays, Z[f'{tag}/qoe_w'], 'cuda')


def run(T, planner, fractions, H, first):
    n = T.n_sample
    sim = BatchedSimulator(T, n, seed=0, worker_num=n).reset()                   # session i plays catalogue entry i
    throughput = torch.full((n,), first, dtype=torch.float64, device='cuda')
    qoe, rebuf, steps = np.zeros(n), np.zeros(n), np.zeros(n, np.int64)
    stalls = 0
    for _ in range(64):                                                           # 64 x 256 decisions: far more than an episode holds
        if planner == 'oracle':
            out = sim.drive(fractions, H, DRIVE_MAX_DECISIONS, throughput, per_tile=False)
        else:
            out = sim.drive_client(fractions, H, DRIVE_MAX_DECISIONS, throughput, window=int(planner[-1]), per_tile=False)
        committed = (out.chunk_size > 0).cpu().numpy()
        q, r = out.qoe.cpu().numpy().astype(np.float64), out.rebuffer_time.cpu().numpy()
        qoe += (q * committed).sum(1)
        rebuf += (r * committed).sum(1)
        steps += committed.sum(1)
        stalls += int(((r > 0) & committed).sum())
        if bool(out.over[:, -1].all().item()):
            break
    else:
        raise SystemExit('an episode did not end')
    return dict(episodes=n, steps=int(steps.sum()), episode_qoe_mean=round(float(qoe.mean()), 4),
                step_qoe_mean=round(float((qoe / np.maximum(steps, 1)).mean()), 5), rebuffered_steps=stalls,
                rebuffer_seconds=round(float(rebuf.sum()), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--fractions', type=float, nargs='+', default=[0.9, 1.3, 2.0, 3.5, 10.0])
    ap.add_argument('--horizon', type=int, default=3)
    ap.add_argument('--throughput', type=float, default=2.0e6, help='the estimate before the first download, bytes/s')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('sim_client_eval needs a ROCm device: nothing is simulated without one')
    Z = np.load(os.path.join(ROOT, 'tests', 'golden', 'env_reference.npz'))
    fractions = torch.tensor(a.fractions, dtype=torch.float64, device='cuda')
    rec = dict(fractions=a.fractions, horizon=a.horizon, first_estimate=a.throughput)
    for tag in ('train_id', 'valid_w3'):
        T = tables(Z, tag)
        rec[tag] = {p: run(T, p, fractions, a.horizon, a.throughput) for p in ('oracle', 'client_w1', 'client_w5')}
    print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
