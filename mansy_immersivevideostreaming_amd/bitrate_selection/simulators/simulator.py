"""Device counterpart of bitrate_selection/simulators/simulator.py:9-114 (+ network.py, buffer.py, hmdtrace.py and utils/qoe.py below
it) for callers that bring their OWN per-tile rate allocation: a rule-based ABR, another action space, a per-tile optimiser, an upper
bound that allocates on the ground-truth viewport.

* `BatchedSimulator` -- n sessions of the `EnvTables` episode catalogue stepped by ONE kernel launch (csrc/sim.hip): tile versions in,
                        tile sizes / qualities / viewport / download + rebuffer time / QoE terms / over flags out, all device tensors.
* `Simulator`        -- one session with the reference's constructor and method names (numpy / Python values in and out).

Both also answer "what would happen if" without moving a session: `lookahead(plans)` downloads K candidate plans of H chunks virtually
from where every session stands (one launch, the state buffer is only read) and `peek(ahead=t)` shows the table rows of the chunks such
plans are made for -- the pattern of the reference's own planner (ExpertEnv.choose_action, envs/expert_env.py:358-422) for arbitrary tile
versions.  `allocate(budgets, weights)` makes such plans: one greedy per-tile allocation under a byte budget per (session, candidate,
chunk), on weights the caller brings or the predicted map, again without moving a session.  `drive(fractions, horizon, decisions,
throughput)` runs that planner closed-loop -- budgets from a throughput estimate, plans, scores, the best plan's first step committed,
the estimate renewed -- for many decisions in one launch.  `lookahead` and `drive` are an oracle (the real trace and the ground-truth
viewport of chunks not yet watched); `lookahead_client` and `drive_client` score the plans as a client that could be deployed has to --
at a throughput estimate made from finished downloads and on the predicted viewport -- and commit on the truth.
`lookahead_schedules` and `drive_schedules` are that client with a budget level PER STEP: every one of the F^H sequences of F levels
over H chunks is a candidate (`schedule_digits` decodes a candidate's index), searched in one launch without materialising its plans.

The session records are the environment's (`mansy_env_init` / `mansy_env_reset`), so sessions walk the catalogue exactly as the
environments of `MANSYVecEnv` do.  A state buffer belongs either to a `MANSYVecEnv` or to a simulator, never both: the simulator keeps no
action history, so the observation rings of such a record are not maintained."""
import ctypes
import types

import numpy as np
import torch

from ..._lib import MansyError, check, lib, ptr, stream_ptr
from ..envs.mansy_env import OBS_LD, EnvTables

N_TILE, N_RATE = 64, 5
MAX_HORIZON, MAX_CANDIDATES = 8, 4096          # MANSY_SIM_MAX_HORIZON, MANSY_SIM_MAX_CANDIDATES of include/mansy_hip.h
DRIVE_MAX_CANDIDATES, DRIVE_MAX_DECISIONS = 64, 256      # MANSY_SIM_DRIVE_MAX_CANDIDATES, MANSY_SIM_DRIVE_MAX_DECISIONS
EST_MAX_WINDOW = 8                                        # MANSY_SIM_EST_MAX_WINDOW: the sample slots of the throughput estimator
VIEWPORTS = {'gt': 0, 'pred': 1}                          # MANSY_SIM_VIEW_GT, MANSY_SIM_VIEW_PRED
NETWORKS = {'trace': 0, 'estimate': 1}                    # MANSY_SIM_NET_TRACE, MANSY_SIM_NET_ESTIMATE
SCHED_MAX_LEVELS = 16                                     # MANSY_SIM_SCHED_MAX_LEVELS: the budget levels of a schedule search


def _choice(name, value, table):
    if not isinstance(value, str) or value not in table:
        raise MansyError(f'{name} must be one of {sorted(table)}, not {value!r}')
    return table[value]


def _sched_shape(F, H):
    """The checks the schedule calls share on the number of levels F and the horizon H; returns K = F^H."""
    for name, x, hi in (('F', F, SCHED_MAX_LEVELS), ('horizon', H, MAX_HORIZON)):
        if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not 1 <= x <= hi:
            raise MansyError(f'{name} must be an integer in 1..{hi}')
    K = int(F) ** int(H)
    if K > MAX_CANDIDATES:
        raise MansyError(f'{F} levels over a horizon of {H} are F^H = {K} schedules: at most {MAX_CANDIDATES} are supported')
    return K


def schedule_digits(F, H):
    """The digit table of a schedule search: int64 tensor [F^H, H] whose row k holds the level candidate k uses at every step,
    (k // F^(H-1-t)) % F at step t -- step 0 is the most significant digit, the candidates are in lexicographic order."""
    K = _sched_shape(F, H)
    place = int(F) ** torch.arange(int(H) - 1, -1, -1, dtype=torch.int64)
    return (torch.arange(K, dtype=torch.int64)[:, None] // place[None, :]) % int(F)


class BatchedSimulator:
    """n sessions; session i (global index `index_offset + i` of `worker_num`) opens catalogue entry (seed + index_offset + i) %
    worker_num first and strides by worker_num on every reset, like environment i of `MANSYVecEnv`.  The returned tensors are this
    object's buffers, overwritten by the next call."""

    def __init__(self, tables, n, seed=0, index_offset=0, worker_num=None):
        self.device = torch.device(tables.device)
        if self.device.type != 'cuda':
            raise MansyError('BatchedSimulator runs on the device: tables on a cuda (ROCm) device are required, there is no CPU path')
        self.tables, self.n = tables, int(n)
        if self.n < 1:
            raise MansyError('BatchedSimulator: n must be >= 1')
        self.worker_num = int(worker_num) if worker_num is not None else self.n
        L = lib()
        self.state = torch.zeros(self.n * L.mansy_env_state_bytes(), dtype=torch.uint8, device=self.device)
        check(L.mansy_env_init(ptr(self.state), self.n, int(index_offset), self.worker_num, int(seed), stream_ptr(self.device)), 'mansy_env_init')
        self._worker = (int(seed) + int(index_offset) + np.arange(self.n, dtype=np.int64)) % self.worker_num      # host mirror of worker_id
        dev = self.device
        f32, f64, u8 = (dict(dtype=t, device=dev) for t in (torch.float32, torch.float64, torch.uint8))
        self.tile_size = torch.zeros(self.n, N_TILE, **f32)
        self.tile_quality = torch.zeros(self.n, N_TILE, **f32)
        self.actual_viewport = torch.zeros(self.n, N_TILE, **u8)
        self.scalars = torch.zeros(self.n, 4, **f64)          # chunk_size, chunk_quality, download_time, rebuffer_time
        self.qoe_parts = torch.zeros(self.n, 4, **f32)        # qoe (unnormalised), qoe1, qoe2 (rebuffer), qoe3
        self.over = torch.ones(self.n, **u8)
        self._peek = dict(next_chunk=torch.zeros(self.n, dtype=torch.int32, device=dev), buffer=torch.zeros(self.n, **f64),
                          size=torch.zeros(self.n, N_RATE, N_TILE, **f32), quality=torch.zeros(self.n, N_RATE, N_TILE, **f32),
                          gt=torch.zeros(self.n, N_TILE, **u8), pred=torch.zeros(self.n, N_TILE, **u8), acc=torch.zeros(self.n, **f64))
        self._out = types.SimpleNamespace(
            tile_size=self.tile_size, tile_quality=self.tile_quality, actual_viewport=self.actual_viewport, scalars=self.scalars,
            chunk_size=self.scalars[:, 0], chunk_quality=self.scalars[:, 1], download_time=self.scalars[:, 2], rebuffer_time=self.scalars[:, 3],
            qoe_parts=self.qoe_parts, qoe=self.qoe_parts[:, 0], qoe1=self.qoe_parts[:, 1], qoe2=self.qoe_parts[:, 2], qoe3=self.qoe_parts[:, 3],
            over=self.over)
        self._peek_ahead = None               # peek(ahead > 0) has buffers of its own, made on first use
        self._look = {}                       # (K, H) -> lookahead()'s buffers and the two namespaces over them
        self._alloc = {}                      # (K, H) -> allocate()'s buffers
        self._drive = {}                      # (K, H, D) -> drive()'s buffers and the two namespaces over them
        self._look_client = {}                # (K, H) -> lookahead_client()'s buffers, its own
        self._drive_client = {}               # (K, H, D) -> drive_client()'s buffers, its own
        self._look_sched = {}                 # (F, H) -> lookahead_schedules()'s buffers
        self._drive_sched = {}                # (F, H, D) -> drive_schedules()'s buffers, its own
        # the throughput estimator of drive_client(): eight sample slots per session (the newest last) and how many are filled
        self.history = torch.zeros(self.n, EST_MAX_WINDOW, **f64)
        self.count = torch.zeros(self.n, dtype=torch.int32, device=dev)

    def reset(self):
        """Every session opens its next catalogue entry at chunk startup_download + 1 with an empty clock (MANSYEnv.reset's
        `Simulator(...)` + `QoEModel(...)`, mansy_env.py:100-115)."""
        n_sample = self.tables.n_sample
        sample = self._worker % n_sample
        bad = sorted(set(int(s) for s in sample) & set(getattr(self.tables, 'unvisitable', ())))
        if bad:
            raise MansyError(f'BatchedSimulator.reset: catalogue entries {bad[:8]} hold no tables (negative slots in `samples`)')
        self._worker = (self._worker + self.worker_num) % n_sample
        obs = torch.empty(self.n, OBS_LD, dtype=torch.float32, device=self.device)     # mansy_env_reset writes an observation: dropped
        check(lib().mansy_env_reset(ctypes.byref(self.tables.c), ptr(self.state), self.n, ptr(obs), stream_ptr(self.device)), 'mansy_env_reset')
        return self

    def reset_estimator(self):
        """Empties the throughput estimator of `drive_client` (`history` and `count` become zeros).  `reset()` and auto_reset leave the
        samples alone: an estimate is carried across episodes, as plain `drive` carries its own."""
        self.history.zero_()
        self.count.zero_()
        return self

    def peek(self, ahead=0):
        """The getters of Simulator for all sessions, as a dict of device tensors: next_chunk i32 [n], buffer f64 [n], size / quality
        f32 [n,5,64] of the next chunk (raw), gt / pred u8 [n,64], acc f64 [n].  Sessions that are over show zeros.
        ahead > 0 (below MAX_HORIZON): the table getters for chunk next_chunk + ahead instead, for a caller that plans over future chunks:
        size, quality, gt, pred, acc and valid u8 [n] (1 iff the session is open and that chunk is one of its own; other rows are
        zeros), in buffers of their own that the next peek(ahead > 0) overwrites."""
        if isinstance(ahead, bool) or not isinstance(ahead, (int, np.integer)) or not 0 <= ahead < MAX_HORIZON:
            raise MansyError(f'ahead must be an integer in 0..{MAX_HORIZON - 1}')
        if ahead > 0:
            if self._peek_ahead is None:
                dev = self.device
                self._peek_ahead = dict(
                    size=torch.zeros(self.n, N_RATE, N_TILE, dtype=torch.float32, device=dev),
                    quality=torch.zeros(self.n, N_RATE, N_TILE, dtype=torch.float32, device=dev),
                    gt=torch.zeros(self.n, N_TILE, dtype=torch.uint8, device=dev), pred=torch.zeros(self.n, N_TILE, dtype=torch.uint8, device=dev),
                    acc=torch.zeros(self.n, dtype=torch.float64, device=dev), valid=torch.zeros(self.n, dtype=torch.uint8, device=dev))
            p = self._peek_ahead
            check(lib().mansy_sim_peek_ahead(ctypes.byref(self.tables.c), ptr(self.state), self.n, int(ahead), ptr(p['size']), ptr(p['quality']),
                                             ptr(p['gt']), ptr(p['pred']), ptr(p['acc']), ptr(p['valid']), stream_ptr(self.device)),
                  'mansy_sim_peek_ahead')
            return p
        p = self._peek
        check(lib().mansy_sim_peek(ctypes.byref(self.tables.c), ptr(self.state), self.n, ptr(p['next_chunk']), ptr(p['buffer']), ptr(p['size']),
                                   ptr(p['quality']), ptr(p['gt']), ptr(p['pred']), ptr(p['acc']), stream_ptr(self.device)), 'mansy_sim_peek')
        return p

    def _look_buffers(self, cache, K, H, per_step):
        """The output buffers of a look-ahead of K candidates x H steps and the two namespaces over them, made on first use."""
        b = cache.get((K, H))
        if b is None:
            dev = self.device
            b = types.SimpleNamespace(total=torch.zeros(self.n, K, dtype=torch.float32, device=dev), steps=torch.zeros(self.n, dtype=torch.int32, device=dev),
                                      best=torch.zeros(self.n, dtype=torch.int32, device=dev), best_total=torch.zeros(self.n, dtype=torch.float32, device=dev),
                                      qoe_parts=None, scalars=None, short=None, full=None)
            b.short = types.SimpleNamespace(total=b.total, steps=b.steps, best=b.best, best_total=b.best_total)
            cache[(K, H)] = b
        if per_step and b.full is None:
            b.qoe_parts = torch.zeros(self.n, K, H, 4, dtype=torch.float32, device=self.device)
            b.scalars = torch.zeros(self.n, K, H, 4, dtype=torch.float64, device=self.device)
            q, s = b.qoe_parts, b.scalars
            b.full = types.SimpleNamespace(total=b.total, steps=b.steps, best=b.best, best_total=b.best_total, qoe_parts=q, qoe=q[..., 0],
                                           qoe1=q[..., 1], qoe2=q[..., 2], qoe3=q[..., 3], scalars=s, chunk_size=s[..., 0],
                                           chunk_quality=s[..., 1], download_time=s[..., 2], rebuffer_time=s[..., 3])
        return b

    def lookahead(self, plans, per_step=True):
        """What would happen if: K candidate plans per session downloaded VIRTUALLY over H chunks from where the session stands, with
        the real trace and the ground-truth viewport (the pattern of ExpertEnv.choose_action, expert_env.py:358-422, for arbitrary tile
        versions).  The sessions do not move: the state buffer is only read.
        plans: int32 cuda tensor [n,K,H,64], contiguous; plans[i,k,t] holds the bitrate VERSION 0..4 of every tile of chunk next_chunk + t
        (values outside are clamped by the kernel), 1 <= K <= MAX_CANDIDATES, 1 <= H <= MAX_HORIZON.
        Returns a namespace of device tensors, without a synchronisation: total f32 [n,K] (float32 sum of the steps' qoe in step order),
        steps i32 [n] = min(H, chunks the session has left; 0 when it is over), best i32 [n] (first candidate with the strictly largest
        total; a NaN never wins) and best_total f32 [n].  per_step adds qoe_parts f32 [n,K,H,4] with the views qoe, qoe1, qoe2, qoe3 and
        scalars f64 [n,K,H,4] with the views chunk_size, chunk_quality, download_time, rebuffer_time; rows t >= steps[i] are zeros.
        The buffers are cached per (K, H) and overwritten by the next call with that shape."""
        if not isinstance(plans, torch.Tensor) or plans.dtype != torch.int32:
            raise MansyError('plans must be an int32 cuda tensor (there is no CPU path)')
        if plans.dim() != 4 or plans.shape[0] != self.n or plans.shape[3] != N_TILE:
            raise MansyError(f'plans must have the shape [{self.n}, K, H, {N_TILE}], not {list(plans.shape)}')
        K, H = int(plans.shape[1]), int(plans.shape[2])
        if not 1 <= K <= MAX_CANDIDATES:
            raise MansyError(f'plans holds K = {K} candidates per session: 1..{MAX_CANDIDATES} are supported')
        if not 1 <= H <= MAX_HORIZON:
            raise MansyError(f'plans holds H = {H} steps per candidate: 1..{MAX_HORIZON} are supported')
        if self.n * K >= 2 ** 31:
            raise MansyError('n * K must stay below 2^31')
        if not plans.is_cuda or plans.device != self.state.device or not plans.is_contiguous():
            raise MansyError(f'plans must be a contiguous int32 cuda tensor on {self.state.device} (there is no CPU path)')
        b = self._look_buffers(self._look, K, H, per_step)
        check(lib().mansy_sim_lookahead(ctypes.byref(self.tables.c), ptr(self.state), self.n, ptr(plans), K, H,
                                        ptr(b.qoe_parts) if per_step else None, ptr(b.scalars) if per_step else None, ptr(b.total),
                                        ptr(b.steps), ptr(b.best), ptr(b.best_total), stream_ptr(self.device)), 'mansy_sim_lookahead')
        return b.full if per_step else b.short

    def allocate(self, budgets, weights=None):
        """Candidate plans from byte budgets (mansy_sim_allocate): for every (session i, candidate k, step t) the tiles of chunk
        next_chunk + t start at version 0 and the upgrade with the largest weight x quality gain per byte that still fits
        budgets[i,k,t] is applied, round by round, until none fits (the lowest tile among equal ratios; an upgrade that costs no bytes
        comes first; include/mansy_hip.h has the definition to the bit).  The sessions do not move: the state buffer is only read.
        budgets: float64 cuda tensor [n,K,H], contiguous, in the units of the manifest sizes (peek()['size']); 1 <= K <= MAX_CANDIDATES,
        1 <= H <= MAX_HORIZON.  weights: float32 cuda tensor [n,H,64], contiguous, the weight of every tile of chunk next_chunk + t
        (shared by the K candidates), or None for the predicted map of that chunk (peek(ahead=t)['pred'] as floats).  A NaN budget, a NaN
        weight or a weight <= 0 upgrades nothing; a budget below the size of version 0 leaves version 0 everywhere.
        Returns a namespace of device tensors, without a synchronisation: plans i32 [n,K,H,64] (goes straight into `lookahead`),
        plan_bytes i32 [n,K,H] (the chunk_size `lookahead` reports for the plan) and steps i32 [n] = min(H, chunks the session has left;
        0 when it is over); rows t >= steps[i] are zeros.  The buffers are cached per (K, H) and overwritten by the next call with that
        shape."""
        if not isinstance(budgets, torch.Tensor) or budgets.dtype != torch.float64:
            raise MansyError('budgets must be a float64 cuda tensor (there is no CPU path)')
        if weights is not None and (not isinstance(weights, torch.Tensor) or weights.dtype != torch.float32):
            raise MansyError('weights must be a float32 cuda tensor or None (there is no CPU path)')
        if budgets.dim() != 3 or budgets.shape[0] != self.n:
            raise MansyError(f'budgets must have the shape [{self.n}, K, H], not {list(budgets.shape)}')
        K, H = int(budgets.shape[1]), int(budgets.shape[2])
        if weights is not None and tuple(weights.shape) != (self.n, H, N_TILE):
            raise MansyError(f'weights must have the shape [{self.n}, H = {H}, {N_TILE}], not {list(weights.shape)}')
        if not 1 <= K <= MAX_CANDIDATES:
            raise MansyError(f'budgets holds K = {K} candidates per session: 1..{MAX_CANDIDATES} are supported')
        if not 1 <= H <= MAX_HORIZON:
            raise MansyError(f'budgets holds H = {H} steps per candidate: 1..{MAX_HORIZON} are supported')
        if self.n * K * H >= 2 ** 31:
            raise MansyError('n * K * H must stay below 2^31')
        for name, x in (('budgets', budgets), ('weights', weights)):
            if x is not None and (not x.is_cuda or x.device != self.state.device or not x.is_contiguous()):
                raise MansyError(f'{name} must be a contiguous {str(x.dtype)[6:]} cuda tensor on {self.state.device} (there is no CPU path)')
        b = self._alloc.get((K, H))
        if b is None:
            dev = self.device
            b = types.SimpleNamespace(plans=torch.zeros(self.n, K, H, N_TILE, dtype=torch.int32, device=dev),
                                      plan_bytes=torch.zeros(self.n, K, H, dtype=torch.int32, device=dev),
                                      steps=torch.zeros(self.n, dtype=torch.int32, device=dev))
            self._alloc[(K, H)] = b
        check(lib().mansy_sim_allocate(ctypes.byref(self.tables.c), ptr(self.state), self.n, ptr(budgets), ptr(weights) if weights is not None else None,
                                       K, H, ptr(b.plans), ptr(b.plan_bytes), ptr(b.steps), stream_ptr(self.device)), 'mansy_sim_allocate')
        return b

    def _drive_buffers(self, cache, K, H, D, per_tile, throughput, **more):
        """The output buffers of a driven run of D decisions and the namespace the call returns (`more`: further fields of it)."""
        b = cache.get((K, H, D))
        if b is None:
            dev = self.device
            q = torch.zeros(self.n, D, 4, dtype=torch.float32, device=dev)
            s = torch.zeros(self.n, D, 4, dtype=torch.float64, device=dev)
            fields = dict(best=torch.zeros(self.n, D, dtype=torch.int32, device=dev), best_total=torch.zeros(self.n, D, dtype=torch.float32, device=dev),
                          qoe_parts=q, qoe=q[..., 0], qoe1=q[..., 1], qoe2=q[..., 2], qoe3=q[..., 3], scalars=s, chunk_size=s[..., 0],
                          chunk_quality=s[..., 1], download_time=s[..., 2], rebuffer_time=s[..., 3],
                          over=torch.ones(self.n, D, dtype=torch.uint8, device=dev), **more)
            b = types.SimpleNamespace(versions=None, short=types.SimpleNamespace(**fields), full=None)
            cache[(K, H, D)] = b
        if per_tile and b.full is None:
            b.versions = torch.zeros(self.n, D, N_TILE, dtype=torch.int32, device=self.device)
            b.full = types.SimpleNamespace(versions=b.versions, **vars(b.short))
        out = b.full if per_tile else b.short
        out.throughput = throughput
        return b, out

    def drive(self, fractions, horizon, decisions, throughput, auto_reset=False, per_tile=True):
        """The planner loop `allocate` -> `lookahead` -> `simulate_download` -> throughput estimate for `decisions` decisions in ONE
        launch (mansy_sim_drive): per decision and session, candidate k plans `horizon` chunks under the byte budget throughput x
        chunk_length x fractions[k] on the predicted maps, the plans are scored, the first step of the best one is committed and
        throughput becomes chunk_size / download_time of that step (unchanged where download_time is not > 0).  Every decision returns
        the bits those calls would (include/mansy_hip.h has the definition), and the sessions move as D committed steps move them.
        fractions: float64 cuda tensor [K], 1 <= K <= DRIVE_MAX_CANDIDATES; 1 <= horizon <= MAX_HORIZON; 1 <= decisions <=
        DRIVE_MAX_DECISIONS; throughput: float64 cuda tensor [n], contiguous, bytes/s, UPDATED IN PLACE.  auto_reset as in
        `simulate_download`; without it a session that ends inside the run gives zeros and over = 1 from then on.
        Returns a namespace of device tensors, without a synchronisation: best i32 [n,D], best_total f32 [n,D], versions i32 [n,D,64]
        (only with per_tile), qoe_parts f32 [n,D,4] with the views qoe, qoe1, qoe2, qoe3, scalars f64 [n,D,4] with the views chunk_size,
        chunk_quality, download_time, rebuffer_time, over u8 [n,D] and throughput (the tensor handed in).  The buffers are cached per
        (K, horizon, decisions) and overwritten by the next call with that shape."""
        if not isinstance(fractions, torch.Tensor) or fractions.dtype != torch.float64:
            raise MansyError('fractions must be a float64 cuda tensor (there is no CPU path)')
        if not isinstance(throughput, torch.Tensor) or throughput.dtype != torch.float64:
            raise MansyError('throughput must be a float64 cuda tensor (there is no CPU path)')
        if fractions.dim() != 1:
            raise MansyError(f'fractions must have the shape [K], not {list(fractions.shape)}')
        if tuple(throughput.shape) != (self.n,):
            raise MansyError(f'throughput must have the shape [{self.n}], not {list(throughput.shape)}')
        K = int(fractions.shape[0])
        if not 1 <= K <= DRIVE_MAX_CANDIDATES:
            raise MansyError(f'fractions holds K = {K} candidates per session: 1..{DRIVE_MAX_CANDIDATES} are supported')
        for name, x, hi in (('horizon', horizon, MAX_HORIZON), ('decisions', decisions, DRIVE_MAX_DECISIONS)):
            if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not 1 <= x <= hi:
                raise MansyError(f'{name} must be an integer in 1..{hi}')
        H, D = int(horizon), int(decisions)
        for name, x in (('fractions', fractions), ('throughput', throughput)):
            if not x.is_cuda or x.device != self.state.device or not x.is_contiguous():
                raise MansyError(f'{name} must be a contiguous float64 cuda tensor on {self.state.device} (there is no CPU path)')
        if auto_reset and getattr(self.tables, 'unvisitable', None):
            raise MansyError('auto_reset walks the whole catalogue, but some of its entries hold no tables (negative slots in `samples`)')
        b, out = self._drive_buffers(self._drive, K, H, D, per_tile, throughput)
        check(lib().mansy_sim_drive(ctypes.byref(self.tables.c), ptr(self.state), self.n, ptr(fractions), K, H, D, ptr(throughput), ptr(out.best),
                                    ptr(out.best_total), ptr(b.versions) if per_tile else None, ptr(out.qoe_parts), ptr(out.scalars),
                                    ptr(out.over), int(bool(auto_reset)), stream_ptr(self.device)), 'mansy_sim_drive')
        return out

    def lookahead_client(self, plans, throughput, viewport='pred', per_step=True):
        """`lookahead` under a client's belief (mansy_sim_lookahead_client): the virtual downloads take chunk_size / throughput[i]
        seconds instead of walking the session's real trace, and the steps are scored on the predicted viewport instead of the ground
        truth.  throughput: float64 cuda tensor [n] (bytes/s; the values are not validated: 0, negative, inf and NaN give what IEEE
        double gives), or None for the real trace.  viewport: 'pred' or 'gt'.  With None and 'gt' the result equals `lookahead`'s.
        plans, per_step and the returned namespaces are `lookahead`'s; the buffers are this method's own, cached per (K, H)."""
        if not isinstance(plans, torch.Tensor) or plans.dtype != torch.int32:
            raise MansyError('plans must be an int32 cuda tensor (there is no CPU path)')
        if throughput is not None and (not isinstance(throughput, torch.Tensor) or throughput.dtype != torch.float64):
            raise MansyError('throughput must be a float64 cuda tensor or None (there is no CPU path)')
        if plans.dim() != 4 or plans.shape[0] != self.n or plans.shape[3] != N_TILE:
            raise MansyError(f'plans must have the shape [{self.n}, K, H, {N_TILE}], not {list(plans.shape)}')
        if throughput is not None and tuple(throughput.shape) != (self.n,):
            raise MansyError(f'throughput must have the shape [{self.n}], not {list(throughput.shape)}')
        K, H = int(plans.shape[1]), int(plans.shape[2])
        if not 1 <= K <= MAX_CANDIDATES:
            raise MansyError(f'plans holds K = {K} candidates per session: 1..{MAX_CANDIDATES} are supported')
        if not 1 <= H <= MAX_HORIZON:
            raise MansyError(f'plans holds H = {H} steps per candidate: 1..{MAX_HORIZON} are supported')
        if self.n * K >= 2 ** 31:
            raise MansyError('n * K must stay below 2^31')
        view = _choice('viewport', viewport, VIEWPORTS)
        for name, x in (('plans', plans), ('throughput', throughput)):
            if x is not None and (not x.is_cuda or x.device != self.state.device or not x.is_contiguous()):
                raise MansyError(f'{name} must be a contiguous {str(x.dtype)[6:]} cuda tensor on {self.state.device} (there is no CPU path)')
        b = self._look_buffers(self._look_client, K, H, per_step)
        check(lib().mansy_sim_lookahead_client(ctypes.byref(self.tables.c), ptr(self.state), self.n, ptr(plans), K, H,
                                               ptr(throughput) if throughput is not None else None, view,
                                               ptr(b.qoe_parts) if per_step else None, ptr(b.scalars) if per_step else None, ptr(b.total),
                                               ptr(b.steps), ptr(b.best), ptr(b.best_total), stream_ptr(self.device)), 'mansy_sim_lookahead_client')
        return b.full if per_step else b.short

    def drive_client(self, fractions, horizon, decisions, throughput, window=5, viewport='pred', network='estimate', auto_reset=False,
                     per_tile=True):
        """`drive` as a client that could be deployed would run it (mansy_sim_drive_client): the candidates are scored by
        `lookahead_client` -- on the predicted viewport ('pred') and, with network='estimate', at the session's current throughput
        estimate instead of the real trace ('trace') -- while the best plan's first step is committed on the truth, as
        `simulate_download` commits it.  After every committed step with download_time > 0 the estimate becomes the harmonic mean of
        the newest min(window, samples so far) values of chunk_size / download_time, 1 <= window <= EST_MAX_WINDOW.  The samples live
        in `self.history` f64 [n,8] (the newest at index 7) and `self.count` i32 [n], which this simulator owns: zeros at construction
        and after `reset_estimator()`; `reset()` and auto_reset leave them alone, so an estimate is carried across episodes (as plain
        `drive` carries its own).  With window=1, viewport='gt', network='trace' the call returns `drive`'s bits.
        The other arguments are `drive`'s.  Returns `drive`'s namespace plus history and count, in buffers of its own, cached per
        (K, horizon, decisions), without a synchronisation."""
        if not isinstance(fractions, torch.Tensor) or fractions.dtype != torch.float64:
            raise MansyError('fractions must be a float64 cuda tensor (there is no CPU path)')
        if not isinstance(throughput, torch.Tensor) or throughput.dtype != torch.float64:
            raise MansyError('throughput must be a float64 cuda tensor (there is no CPU path)')
        if fractions.dim() != 1:
            raise MansyError(f'fractions must have the shape [K], not {list(fractions.shape)}')
        if tuple(throughput.shape) != (self.n,):
            raise MansyError(f'throughput must have the shape [{self.n}], not {list(throughput.shape)}')
        K = int(fractions.shape[0])
        if not 1 <= K <= DRIVE_MAX_CANDIDATES:
            raise MansyError(f'fractions holds K = {K} candidates per session: 1..{DRIVE_MAX_CANDIDATES} are supported')
        for name, x, hi in (('horizon', horizon, MAX_HORIZON), ('decisions', decisions, DRIVE_MAX_DECISIONS), ('window', window, EST_MAX_WINDOW)):
            if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not 1 <= x <= hi:
                raise MansyError(f'{name} must be an integer in 1..{hi}')
        H, D = int(horizon), int(decisions)
        view, net = _choice('viewport', viewport, VIEWPORTS), _choice('network', network, NETWORKS)
        for name, x in (('fractions', fractions), ('throughput', throughput)):
            if not x.is_cuda or x.device != self.state.device or not x.is_contiguous():
                raise MansyError(f'{name} must be a contiguous float64 cuda tensor on {self.state.device} (there is no CPU path)')
        if auto_reset and getattr(self.tables, 'unvisitable', None):
            raise MansyError('auto_reset walks the whole catalogue, but some of its entries hold no tables (negative slots in `samples`)')
        b, out = self._drive_buffers(self._drive_client, K, H, D, per_tile, throughput, history=self.history, count=self.count)
        check(lib().mansy_sim_drive_client(ctypes.byref(self.tables.c), ptr(self.state), self.n, ptr(fractions), K, H, D, ptr(throughput), net, view,
                                           int(window), ptr(self.history), ptr(self.count), ptr(out.best), ptr(out.best_total),
                                           ptr(b.versions) if per_tile else None, ptr(out.qoe_parts), ptr(out.scalars), ptr(out.over),
                                           int(bool(auto_reset)), stream_ptr(self.device)), 'mansy_sim_drive_client')
        return out

    def _sched_arguments(self, levels, horizon, throughput):
        """The argument checks `lookahead_schedules` and `drive_schedules` share; returns F, H and K = F^H."""
        if not isinstance(levels, torch.Tensor) or levels.dtype != torch.float64:
            raise MansyError('levels must be a float64 cuda tensor (there is no CPU path)')
        if not isinstance(throughput, torch.Tensor) or throughput.dtype != torch.float64:
            raise MansyError('throughput must be a float64 cuda tensor (there is no CPU path)')
        if levels.dim() != 1:
            raise MansyError(f'levels must have the shape [F], not {list(levels.shape)}')
        if tuple(throughput.shape) != (self.n,):
            raise MansyError(f'throughput must have the shape [{self.n}], not {list(throughput.shape)}')
        F = int(levels.shape[0])
        if not 1 <= F <= SCHED_MAX_LEVELS:
            raise MansyError(f'levels holds F = {F} budget levels: 1..{SCHED_MAX_LEVELS} are supported')
        K = _sched_shape(F, horizon)
        if self.n * K >= 2 ** 31:
            raise MansyError('n * F^H must stay below 2^31')
        return F, int(horizon), K

    def lookahead_schedules(self, levels, horizon, throughput, network='estimate', viewport='pred', per_leaf=True):
        """The client's look-ahead over BUDGET SCHEDULES (mansy_sim_lookahead_schedules): candidate k of the K = F^horizon candidates
        plans chunk next_chunk + t under the byte budget throughput[i] x chunk_length x levels[digit_t(k)], its digits being row k of
        `schedule_digits(F, horizon)`.  The call returns the bits of `allocate` on those budgets [n,K,H] followed by
        `lookahead_client(plans, throughput if network == 'estimate' else None, viewport, per_step=False)`, without making the K x H
        plans: a schedule's plan for a chunk depends on its level there alone, so F x H allocations serve all of them.  The sessions
        do not move.
        levels: float64 cuda tensor [F], 1 <= F <= SCHED_MAX_LEVELS, F^horizon <= MAX_CANDIDATES; throughput: float64 cuda tensor [n].
        Returns a namespace of device tensors, without a synchronisation: total f32 [n,K] (only with per_leaf), steps i32 [n], best i32
        [n], best_total f32 [n], level_plans i32 [n,F,H,64] and level_bytes i32 [n,F,H] (the plan and its size of every schedule that
        uses level f at step t; rows t >= steps[i] are zeros).  Where steps[i] < horizon the schedules that share their first steps[i]
        digits tie and the first wins: the trailing digits of best are 0.  The buffers are cached per (F, horizon)."""
        F, H, K = self._sched_arguments(levels, horizon, throughput)
        view, net = _choice('viewport', viewport, VIEWPORTS), _choice('network', network, NETWORKS)
        for name, x in (('levels', levels), ('throughput', throughput)):
            if not x.is_cuda or x.device != self.state.device or not x.is_contiguous():
                raise MansyError(f'{name} must be a contiguous float64 cuda tensor on {self.state.device} (there is no CPU path)')
        b = self._look_sched.get((F, H))
        if b is None:
            dev = self.device
            short = types.SimpleNamespace(steps=torch.zeros(self.n, dtype=torch.int32, device=dev), best=torch.zeros(self.n, dtype=torch.int32, device=dev),
                                          best_total=torch.zeros(self.n, dtype=torch.float32, device=dev),
                                          level_plans=torch.zeros(self.n, F, H, N_TILE, dtype=torch.int32, device=dev),
                                          level_bytes=torch.zeros(self.n, F, H, dtype=torch.int32, device=dev))
            b = types.SimpleNamespace(total=None, short=short, full=None)
            self._look_sched[(F, H)] = b
        if per_leaf and b.full is None:
            b.total = torch.zeros(self.n, K, dtype=torch.float32, device=self.device)
            b.full = types.SimpleNamespace(total=b.total, **vars(b.short))
        out = b.full if per_leaf else b.short
        check(lib().mansy_sim_lookahead_schedules(ctypes.byref(self.tables.c), ptr(self.state), self.n, ptr(levels), F, H, ptr(throughput), net, view,
                                                  ptr(out.level_plans), ptr(out.level_bytes), ptr(b.total) if per_leaf else None, ptr(out.steps),
                                                  ptr(out.best), ptr(out.best_total), stream_ptr(self.device)), 'mansy_sim_lookahead_schedules')
        return out

    def drive_schedules(self, levels, horizon, decisions, throughput, window=5, viewport='pred', network='estimate', auto_reset=False,
                        per_tile=True):
        """`drive_client` with the schedule search in the place of its K candidates (mansy_sim_drive_schedules): per decision and
        session `lookahead_schedules` at the current estimate picks the best of the F^horizon budget schedules, the plan of its FIRST
        level for the next chunk is committed on the truth and the estimator is renewed, all as `drive_client` does it, auto_reset and
        the estimator carried across episodes included.  With horizon=1 the call returns `drive_client(levels, 1, ...)`'s bits.
        levels: float64 cuda tensor [F] as in `lookahead_schedules`; the other arguments are `drive_client`'s.  Returns `drive_client`'s
        namespace in buffers of its own, cached per (F, horizon, decisions), without a synchronisation: best i32 [n,D] is the schedule's
        index, and first_level i64 [n,D] = best // F^(horizon-1) the level it commits."""
        F, H, K = self._sched_arguments(levels, horizon, throughput)
        for name, x, hi in (('decisions', decisions, DRIVE_MAX_DECISIONS), ('window', window, EST_MAX_WINDOW)):
            if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not 1 <= x <= hi:
                raise MansyError(f'{name} must be an integer in 1..{hi}')
        D = int(decisions)
        view, net = _choice('viewport', viewport, VIEWPORTS), _choice('network', network, NETWORKS)
        for name, x in (('levels', levels), ('throughput', throughput)):
            if not x.is_cuda or x.device != self.state.device or not x.is_contiguous():
                raise MansyError(f'{name} must be a contiguous float64 cuda tensor on {self.state.device} (there is no CPU path)')
        if auto_reset and getattr(self.tables, 'unvisitable', None):
            raise MansyError('auto_reset walks the whole catalogue, but some of its entries hold no tables (negative slots in `samples`)')
        b, out = self._drive_buffers(self._drive_sched, F, H, D, per_tile, throughput, history=self.history, count=self.count)
        check(lib().mansy_sim_drive_schedules(ctypes.byref(self.tables.c), ptr(self.state), self.n, ptr(levels), F, H, D, ptr(throughput), net, view,
                                              int(window), ptr(self.history), ptr(self.count), ptr(out.best), ptr(out.best_total),
                                              ptr(b.versions) if per_tile else None, ptr(out.qoe_parts), ptr(out.scalars), ptr(out.over),
                                              int(bool(auto_reset)), stream_ptr(self.device)), 'mansy_sim_drive_schedules')
        out.first_level = out.best.long() // F ** (H - 1)
        return out

    def simulate_download(self, tile_rates, auto_reset=False, validate=False):
        """tile_rates: int32 cuda tensor [n,64], bitrate VERSION 0..4 per tile (values outside are clamped by the kernel; validate=True
        raises instead, at the cost of one synchronisation).  Returns a namespace of device tensors: tile_size, tile_quality [n,64] f32,
        actual_viewport [n,64] u8, chunk_size, chunk_quality, download_time, rebuffer_time [n] f64 (columns of `scalars` [n,4]),
        qoe, qoe1, qoe2, qoe3 [n] f32 (columns of `qoe_parts` [n,4]; qoe is the unnormalised one), over [n] u8.  auto_reset: a session
        that ends opens its next catalogue entry, as the vector environment does; without it a finished session returns zeros and
        over = 1 until `reset()`."""
        if not isinstance(tile_rates, torch.Tensor) or not tile_rates.is_cuda or tile_rates.dtype != torch.int32:
            raise MansyError('tile_rates must be an int32 cuda tensor (there is no CPU path)')
        if tuple(tile_rates.shape) != (self.n, N_TILE) or not tile_rates.is_contiguous() or tile_rates.device != self.state.device:
            raise MansyError(f'tile_rates must be a contiguous [{self.n}, {N_TILE}] tensor on {self.state.device}')
        if validate and bool(((tile_rates < 0) | (tile_rates > N_RATE - 1)).any().item()):
            raise MansyError(f'tile_rates holds a version outside 0..{N_RATE - 1}')
        if auto_reset and getattr(self.tables, 'unvisitable', None):
            raise MansyError('auto_reset walks the whole catalogue, but some of its entries hold no tables (negative slots in `samples`)')
        check(lib().mansy_sim_download(ctypes.byref(self.tables.c), ptr(self.state), self.n, ptr(tile_rates), ptr(self.tile_size),
                                       ptr(self.tile_quality), ptr(self.actual_viewport), ptr(self.scalars), ptr(self.qoe_parts),
                                       ptr(self.over), int(bool(auto_reset)), stream_ptr(self.device)), 'mansy_sim_download')
        return self._out


class Simulator:
    """Drop-in single session (reference constructor signature, simulator.py:15): the viewport trace of (video, user), the network trace
    `trace` and the manifest of `video`, downloaded chunk by chunk with the caller's tile rates.  Values come back as the reference's
    types (float32 arrays, Python numbers); each call is one launch and one small copy to the host -- use `BatchedSimulator` for
    throughput.  There is no CPU path: device='cpu' raises MansyError."""

    def __init__(self, config, dataset, video, user, network_dataset, trace, startup_download, trace_scale=None, device='cuda'):
        if torch.device(device).type != 'cuda':
            raise MansyError('Simulator runs on the device: a cuda (ROCm) device is required, there is no CPU path')
        self.config = config
        self.startup_download = int(startup_download)
        arrays, ids = EnvTables.arrays_from_dataset(config, dataset, network_dataset, None, [(1, 1, 1)], samples=[(0, 0, 0, 0)],
                                                    lists=([video], [user], [trace]), trace_scale=trace_scale)
        self.video_length = int(arrays['video_len'][0])
        self.start_chunk = int(arrays['vp_start'][0])
        self.end_chunk = min(int(arrays['vp_end'][0]), self.video_length - 1)
        self.chunk_num = self.end_chunk - self.start_chunk + 1
        if self.startup_download + 1 < self.start_chunk:                       # simulator.py:45
            raise MansyError(f'the viewport trace starts at chunk {self.start_chunk}, after startup_download + 1 = {self.startup_download + 1}')
        self.tables = EnvTables(arrays, [(1, 1, 1)], device, video_rates=config.video_rates, startup_download=self.startup_download,
                                chunk_length=config.chunk_length, max_size=config.max_size, max_throughput=config.max_throughput, ids=ids)
        self.device = self.tables.device
        self._sim = BatchedSimulator(self.tables, 1, seed=0, index_offset=0, worker_num=1)
        self._rates = torch.zeros(1, N_TILE, dtype=torch.int32, device=self.device)
        self.reset()

    # ---- getters (simulator.py:48-86); chunk=None is the next chunk, read from the device
    def _peek(self):
        if self.next_chunk > self.end_chunk:
            raise MansyError(f'the session is over (next chunk {self.next_chunk} > end chunk {self.end_chunk})')
        return self._sim.peek()

    def get_next_chunk_size(self, chunk=None):
        if chunk is None:
            return self._peek()['size'][0].cpu().numpy()
        return self.tables.host['size'][0, int(chunk)].astype(np.float32)

    def get_chunk_num(self):
        return self.chunk_num

    def get_next_chunk_quality(self, chunk=None):
        if chunk is None:
            return self._peek()['quality'][0].cpu().numpy()
        return self.tables.host['quality'][0, int(chunk)].astype(np.float32)

    def get_next_chunk_info(self, chunk=None):
        chunk = self.next_chunk if chunk is None else int(chunk)
        return self.tables.host['size'][0, chunk].tolist(), self.tables.host['quality'][0, chunk].tolist()

    def get_viewport(self, chunk=None, flatten=True):
        if chunk is None:
            p = self._peek()
            gt, pred, acc = p['gt'][0].cpu().numpy(), p['pred'][0].cpu().numpy(), np.float64(p['acc'][0].item())
        else:
            j = int(chunk) - self.start_chunk
            if j < 0:
                raise MansyError(f'chunk {chunk} lies before the viewport trace (it starts at chunk {self.start_chunk})')
            h = self.tables.host
            gt, pred, acc = h['vp_gt'][0, j], h['vp_pred'][0, j], np.float64(h['vp_acc'][0, j])
        gt, pred = np.array(gt, dtype=np.float32), np.array(pred, dtype=np.float32)
        if not flatten:
            gt = gt.reshape(self.config.tile_num_height, self.config.tile_num_width)
            pred = pred.reshape(self.config.tile_num_height, self.config.tile_num_width)
        return gt, pred, acc

    def get_buffer_size(self):
        if self.next_chunk > self.end_chunk:                   # the device shows zeros for a finished session: the host copy serves it
            return self._buffer
        return float(self._sim.peek()['buffer'][0].item())

    def get_next_chunk(self):
        return self.next_chunk

    def simulate_download(self, tile_rates):
        """Given the bitrate version of each tile, download the next chunk (simulator.py:88-108).  Returns the reference's 8-tuple:
        tile sizes, tile qualities (float32 [64]), chunk_size (int), chunk_quality (float; the reference's is an int where the manifest
        stores integers), download_time, rebuffer_time (float), actual_viewport (uint8 [64]), over (bool)."""
        if self.next_chunk > self.end_chunk:
            raise MansyError(f'the session is over (next chunk {self.next_chunk} > end chunk {self.end_chunk})')
        rates = np.asarray(tile_rates).reshape(-1)
        if rates.size != N_TILE or (rates < 0).any() or (rates > N_RATE - 1).any():
            raise MansyError(f'tile_rates must hold {N_TILE} versions in 0..{N_RATE - 1}')
        self._rates.copy_(torch.from_numpy(rates.astype(np.int32)).view(1, N_TILE))
        out = self._sim.simulate_download(self._rates)
        sc = out.scalars[0].cpu().numpy()
        download_time, rebuffer_time = float(sc[2]), float(sc[3])
        # PlaybackBuffer.push_chunk (buffer.py:8-15) on the host copy that get_buffer_size() serves after the last chunk too
        chunk_length = self.config.chunk_length
        self._buffer = chunk_length if download_time > self._buffer else self._buffer - download_time + chunk_length
        self.next_chunk += 1
        over = bool(out.over[0].item())
        assert over == (self.next_chunk > self.end_chunk)
        return (out.tile_size[0].cpu().numpy(), out.tile_quality[0].cpu().numpy(), int(sc[0]), float(sc[1]), download_time, rebuffer_time,
                out.actual_viewport[0].cpu().numpy(), over)

    def lookahead(self, plans):
        """K candidate plans of H chunks each, downloaded virtually from where the session stands (BatchedSimulator.lookahead); the
        session does not move.  plans: array-like [K,H,64] of versions 0..4.  Returns a namespace: total float32 [K], steps (int; the
        chunks of the horizon the session still has, 0 when it is over), best (int; first candidate with the largest total),
        qoe float32 [K,H,4] = qoe, qoe1, qoe2, qoe3 and scalars float64 [K,H,4] = chunk_size, chunk_quality, download_time, rebuffer_time
        of every virtual step (rows t >= steps are zeros)."""
        try:
            p = np.asarray(plans)
        except Exception as e:
            raise MansyError(f'plans must be array-like [K, H, {N_TILE}]: {e}')
        if p.ndim != 3 or p.shape[2] != N_TILE or p.dtype.kind not in 'iu' or not 1 <= p.shape[0] <= MAX_CANDIDATES or not 1 <= p.shape[1] <= MAX_HORIZON:
            raise MansyError(f'plans must be integers [K, H, {N_TILE}] with 1 <= K <= {MAX_CANDIDATES} and 1 <= H <= {MAX_HORIZON}')
        if (p < 0).any() or (p > N_RATE - 1).any():
            raise MansyError(f'plans must hold versions in 0..{N_RATE - 1}')
        dev_plans = torch.from_numpy(np.ascontiguousarray(p, dtype=np.int32)[None]).to(self.device)
        out = self._sim.lookahead(dev_plans)
        return types.SimpleNamespace(total=out.total[0].cpu().numpy(), steps=int(out.steps[0].item()), best=int(out.best[0].item()),
                                     qoe=out.qoe_parts[0].cpu().numpy(), scalars=out.scalars[0].cpu().numpy())

    def allocate(self, budgets, weights=None):
        """K candidate plans of H chunks made from byte budgets (BatchedSimulator.allocate); the session does not move.  budgets:
        array-like [K,H] of numbers, weights: array-like [H,64] or None (the predicted maps).  Returns a namespace: plans int32
        [K,H,64], plan_bytes int32 [K,H] and steps (int; rows t >= steps are zeros)."""
        try:
            b = np.asarray(budgets)
            w = None if weights is None else np.asarray(weights)
        except Exception as e:
            raise MansyError(f'budgets must be array-like [K, H] and weights [H, {N_TILE}]: {e}')
        if b.ndim != 2 or b.dtype.kind not in 'fiu' or not 1 <= b.shape[0] <= MAX_CANDIDATES or not 1 <= b.shape[1] <= MAX_HORIZON:
            raise MansyError(f'budgets must be numbers [K, H] with 1 <= K <= {MAX_CANDIDATES} and 1 <= H <= {MAX_HORIZON}')
        if w is not None and (w.dtype.kind not in 'fiu' or w.shape != (b.shape[1], N_TILE)):
            raise MansyError(f'weights must be numbers [H = {b.shape[1]}, {N_TILE}] or None')
        dev_b = torch.from_numpy(np.ascontiguousarray(b, dtype=np.float64)[None]).to(self.device)
        dev_w = None if w is None else torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32)[None]).to(self.device)
        out = self._sim.allocate(dev_b, dev_w)
        return types.SimpleNamespace(plans=out.plans[0].cpu().numpy(), plan_bytes=out.plan_bytes[0].cpu().numpy(), steps=int(out.steps[0].item()))

    def drive(self, fractions, horizon, decisions, throughput):
        """`decisions` decisions of the budget planner on this session in one launch (BatchedSimulator.drive without auto_reset):
        fractions array-like [K] of numbers, throughput a number (bytes/s).  Returns the new throughput estimate as a float.  The
        decisions' outputs stay in `self.driven`, a namespace of numpy arrays: best [D], best_total [D], versions [D,64], qoe [D,4] =
        qoe, qoe1, qoe2, qoe3, scalars [D,4] = chunk_size, chunk_quality, download_time, rebuffer_time, over [D] and steps (int; the
        decisions that committed a chunk -- rows after the session's end are zeros with over = 1)."""
        if self.next_chunk > self.end_chunk:
            raise MansyError(f'the session is over (next chunk {self.next_chunk} > end chunk {self.end_chunk})')
        try:
            f = np.asarray(fractions)
            thr = float(throughput)
        except Exception as e:
            raise MansyError(f'fractions must be array-like [K] and throughput a number: {e}')
        if f.ndim != 1 or f.dtype.kind not in 'fiu' or not 1 <= f.shape[0] <= DRIVE_MAX_CANDIDATES:
            raise MansyError(f'fractions must be numbers [K] with 1 <= K <= {DRIVE_MAX_CANDIDATES}')
        dev_f = torch.from_numpy(np.ascontiguousarray(f, dtype=np.float64)).to(self.device)
        dev_thr = torch.tensor([thr], dtype=torch.float64, device=self.device)
        out = self._sim.drive(dev_f, horizon, decisions, dev_thr)
        self._mirror_driven(out, int(decisions))
        return float(dev_thr[0].item())

    def lookahead_client(self, plans, throughput, viewport='pred'):
        """`lookahead` under a client's belief (BatchedSimulator.lookahead_client): throughput a number (bytes/s) or None for the real
        trace, viewport 'pred' or 'gt'.  Returns `lookahead`'s namespace."""
        try:
            p = np.asarray(plans)
            thr = None if throughput is None else float(throughput)
        except Exception as e:
            raise MansyError(f'plans must be array-like [K, H, {N_TILE}] and throughput a number or None: {e}')
        if p.ndim != 3 or p.shape[2] != N_TILE or p.dtype.kind not in 'iu' or not 1 <= p.shape[0] <= MAX_CANDIDATES or not 1 <= p.shape[1] <= MAX_HORIZON:
            raise MansyError(f'plans must be integers [K, H, {N_TILE}] with 1 <= K <= {MAX_CANDIDATES} and 1 <= H <= {MAX_HORIZON}')
        if (p < 0).any() or (p > N_RATE - 1).any():
            raise MansyError(f'plans must hold versions in 0..{N_RATE - 1}')
        _choice('viewport', viewport, VIEWPORTS)
        dev_plans = torch.from_numpy(np.ascontiguousarray(p, dtype=np.int32)[None]).to(self.device)
        dev_thr = None if thr is None else torch.tensor([thr], dtype=torch.float64, device=self.device)
        out = self._sim.lookahead_client(dev_plans, dev_thr, viewport)
        return types.SimpleNamespace(total=out.total[0].cpu().numpy(), steps=int(out.steps[0].item()), best=int(out.best[0].item()),
                                     qoe=out.qoe_parts[0].cpu().numpy(), scalars=out.scalars[0].cpu().numpy())

    def drive_client(self, fractions, horizon, decisions, throughput, window=5, viewport='pred', network='estimate'):
        """`drive` as a deployable client runs it (BatchedSimulator.drive_client without auto_reset).  Returns the new estimate as a
        float; the decisions' outputs stay in `self.driven` as `drive` leaves them, plus history float64 [8] (the newest sample last)
        and count (int).  `reset()` empties the estimator."""
        if self.next_chunk > self.end_chunk:
            raise MansyError(f'the session is over (next chunk {self.next_chunk} > end chunk {self.end_chunk})')
        try:
            f = np.asarray(fractions)
            thr = float(throughput)
        except Exception as e:
            raise MansyError(f'fractions must be array-like [K] and throughput a number: {e}')
        if f.ndim != 1 or f.dtype.kind not in 'fiu' or not 1 <= f.shape[0] <= DRIVE_MAX_CANDIDATES:
            raise MansyError(f'fractions must be numbers [K] with 1 <= K <= {DRIVE_MAX_CANDIDATES}')
        dev_f = torch.from_numpy(np.ascontiguousarray(f, dtype=np.float64)).to(self.device)
        dev_thr = torch.tensor([thr], dtype=torch.float64, device=self.device)
        out = self._sim.drive_client(dev_f, horizon, decisions, dev_thr, window=window, viewport=viewport, network=network)
        self._mirror_driven(out, int(decisions))
        self.driven.history, self.driven.count = out.history[0].cpu().numpy(), int(out.count[0].item())
        return float(dev_thr[0].item())

    def _levels(self, levels, horizon, throughput):
        """The array arguments of the two schedule calls as device tensors: levels [F] and the estimate [1]."""
        try:
            f = np.asarray(levels)
            thr = float(throughput)
        except Exception as e:
            raise MansyError(f'levels must be array-like [F] and throughput a number: {e}')
        if f.ndim != 1 or f.dtype.kind not in 'fiu' or not 1 <= f.shape[0] <= SCHED_MAX_LEVELS:
            raise MansyError(f'levels must be numbers [F] with 1 <= F <= {SCHED_MAX_LEVELS}')
        _sched_shape(int(f.shape[0]), horizon)
        return (torch.from_numpy(np.ascontiguousarray(f, dtype=np.float64)).to(self.device),
                torch.tensor([thr], dtype=torch.float64, device=self.device))

    def lookahead_schedules(self, levels, horizon, throughput, network='estimate', viewport='pred'):
        """The F^horizon budget schedules of `levels` (array-like [F] of numbers) scored from where the session stands
        (BatchedSimulator.lookahead_schedules); the session does not move.  throughput: a number (bytes/s).  Returns a namespace: total
        float32 [F^horizon], steps (int), best (int; `schedule_digits` decodes it), best_total (float), level_plans int32 [F,H,64] and
        level_bytes int32 [F,H] (rows t >= steps are zeros)."""
        _choice('viewport', viewport, VIEWPORTS), _choice('network', network, NETWORKS)
        dev_f, dev_thr = self._levels(levels, horizon, throughput)
        out = self._sim.lookahead_schedules(dev_f, horizon, dev_thr, network=network, viewport=viewport)
        return types.SimpleNamespace(total=out.total[0].cpu().numpy(), steps=int(out.steps[0].item()), best=int(out.best[0].item()),
                                     best_total=float(out.best_total[0].item()), level_plans=out.level_plans[0].cpu().numpy(),
                                     level_bytes=out.level_bytes[0].cpu().numpy())

    def drive_schedules(self, levels, horizon, decisions, throughput, window=5, viewport='pred', network='estimate'):
        """`drive_client` over budget schedules (BatchedSimulator.drive_schedules without auto_reset): levels array-like [F] of numbers.
        Returns the new estimate as a float; the decisions' outputs stay in `self.driven` as `drive_client` leaves them (best holds the
        schedule's index), plus first_level int64 [D]."""
        if self.next_chunk > self.end_chunk:
            raise MansyError(f'the session is over (next chunk {self.next_chunk} > end chunk {self.end_chunk})')
        dev_f, dev_thr = self._levels(levels, horizon, throughput)
        out = self._sim.drive_schedules(dev_f, horizon, decisions, dev_thr, window=window, viewport=viewport, network=network)
        self._mirror_driven(out, int(decisions))
        self.driven.history, self.driven.count = out.history[0].cpu().numpy(), int(out.count[0].item())
        self.driven.first_level = out.first_level[0].cpu().numpy()
        return float(dev_thr[0].item())

    def _mirror_driven(self, out, decisions):
        """The host mirrors after a driven run, as simulate_download keeps them, up to the session's end; fills `self.driven`."""
        sc, over = out.scalars[0].cpu().numpy(), out.over[0].cpu().numpy()
        chunk_length, steps = self.config.chunk_length, 0
        for d in range(decisions):
            if self.next_chunk > self.end_chunk:
                break
            download_time = float(sc[d, 2])
            self._buffer = chunk_length if download_time > self._buffer else self._buffer - download_time + chunk_length
            self.next_chunk += 1
            steps += 1
            assert bool(over[d]) == (self.next_chunk > self.end_chunk)
        self.driven = types.SimpleNamespace(best=out.best[0].cpu().numpy(), best_total=out.best_total[0].cpu().numpy(),
                                            versions=out.versions[0].cpu().numpy(), qoe=out.qoe_parts[0].cpu().numpy(), scalars=sc, over=over,
                                            steps=steps)

    def reset(self):
        """Restarts the SAME session at chunk startup_download + 1 with an empty clock and the start-up buffer, as a freshly constructed
        reference Simulator would.  (The reference's own reset(), simulator.py:110-114, sets next_chunk = startup_download -- one chunk
        earlier than its constructor does; its environment never relies on it, it builds a new Simulator per episode.)"""
        self._sim.reset()                      # a one-entry catalogue: the next entry is this session again
        self._sim.reset_estimator()            # and drive_client's samples belong to the session that ended
        self.next_chunk = self.startup_download + 1
        self._buffer = self.config.chunk_length * 3
