#!/usr/bin/env python3
"""Rate of the simulator's what-if (mansy_sim_lookahead: K candidate plans of H chunks per session, scored from the sessions' records
without moving them) in virtual candidate-steps/s, next to the same work done with the interface that existed before it: the n records
repeated K times into a state buffer of n * K records (the copy is part of the time) and H mansy_sim_download launches on that buffer.
Synthetic bench-shaped tables, sessions a few chunks into their episodes.  Two output sets are timed: `per_step` (the QoE terms and the
download scalars of every virtual step: qoe_parts + scalars on both sides) and `totals` (the look-ahead returns total / best only; the
replicate-and-step side still has to write each step's qoe_parts, and the sum over the steps it would need is not even counted).
Event-timed blocks of launches after a warm-up, the variants alternating block by block; the median block is reported with the spread
(min .. max of the blocks).  One launch runs for milliseconds, so the host's enqueue cost does not show."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mansy_immersivevideostreaming_amd._lib import check, lib, ptr, stream_ptr  # noqa: E402
from mansy_immersivevideostreaming_amd.bitrate_selection.envs.mansy_env import EnvTables  # noqa: E402
from mansy_immersivevideostreaming_amd.bitrate_selection.simulators import BatchedSimulator  # noqa: E402


def timed(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=4096)
    ap.add_argument('--K', type=int, default=64)
    ap.add_argument('--H', type=int, default=4)
    ap.add_argument('--launches', type=int, default=10, help='look-aheads per timed block')
    ap.add_argument('--blocks', type=int, default=9)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('sim_lookahead_bench needs a ROCm device: nothing is measured without one')
    n, K, H = a.n, a.K, a.H
    T = EnvTables.synthetic('cuda', seed=5, train_identifier_reward=False)
    rs = np.random.RandomState(0)
    sim = BatchedSimulator(T, n, seed=0).reset()
    for _ in range(10):
        sim.simulate_download(torch.from_numpy(rs.randint(0, 5, size=(n, 64)).astype(np.int32)).cuda())
    plans = torch.from_numpy(rs.randint(0, 5, size=(n, K, H, 64)).astype(np.int32)).cuda()
    # the replicate-and-step side: its own n * K records and outputs, the versions regrouped per step (not timed)
    L, Tc, st = lib(), ctypes.byref(T.c), stream_ptr()
    nb = L.mansy_env_state_bytes()
    big = torch.zeros(n * K * nb, dtype=torch.uint8, device='cuda')
    by_step = plans.permute(2, 0, 1, 3).contiguous()
    qoe_parts = torch.zeros(H, n * K, 4, dtype=torch.float32, device='cuda')
    scalars = torch.zeros(H, n * K, 4, dtype=torch.float64, device='cuda')
    over = torch.zeros(n * K, dtype=torch.uint8, device='cuda')

    def replicate_and_step(with_scalars):
        big.view(n, K, nb).copy_(sim.state.view(n, 1, nb).expand(n, K, nb))
        for t in range(H):
            check(L.mansy_sim_download(Tc, ptr(big), n * K, ptr(by_step[t]), None, None, None, ptr(scalars[t]) if with_scalars else None,
                                       ptr(qoe_parts[t]), ptr(over), 0, st), 'mansy_sim_download')

    fns = {('lookahead', 'per_step'): lambda: sim.lookahead(plans), ('lookahead', 'totals'): lambda: sim.lookahead(plans, per_step=False),
           ('replicate_and_step', 'per_step'): lambda: replicate_and_step(True), ('replicate_and_step', 'totals'): lambda: replicate_and_step(False)}
    for fn in fns.values():
        timed(fn, a.warmup)
    # both sides computed the same steps: the bits agree before anything is timed
    out = sim.lookahead(plans)
    replicate_and_step(True)
    assert torch.equal(out.qoe_parts.view(torch.int32), qoe_parts.view(H, n, K, 4).permute(1, 2, 0, 3).contiguous().view(torch.int32))
    assert torch.equal(out.scalars.view(torch.int64), scalars.view(H, n, K, 4).permute(1, 2, 0, 3).contiguous().view(torch.int64))
    ms = {k: [] for k in fns}
    for _ in range(a.blocks):
        for k, fn in fns.items():
            ms[k].append(timed(fn, a.launches))
    work = n * K * H
    rec = dict(n=n, K=K, H=H, candidate_steps_per_launch=work, launches_per_block=a.launches, blocks=a.blocks, device=torch.cuda.get_device_name(0))
    for (who, what), x in ms.items():
        med = statistics.median(x)
        rec.setdefault(who, {})[what] = dict(ms_median=round(med, 4), ms_min=round(min(x), 4), ms_max=round(max(x), 4),
                                             spread_pct=round((max(x) - min(x)) / med * 100, 2),
                                             candidate_steps_per_s=round(work / med * 1e3))
    for what in ('per_step', 'totals'):
        rec[f'speedup_{what}'] = round(rec['replicate_and_step'][what]['ms_median'] / rec['lookahead'][what]['ms_median'], 3)
    print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
