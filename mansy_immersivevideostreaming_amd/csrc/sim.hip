// Batched streaming simulator: the environment step of csrc/env.hip with the tile-rate allocation taken out.  The caller hands in
// the bitrate VERSION of every tile, so any allocator (rule-based ABR, another action space, a per-tile optimiser, an upper bound on
// the ground-truth viewport) can drive the Jin2022 x 4G sessions.  One 64-lane wavefront per session, lane = tile.
// Reference semantics:
//   Simulator.simulate_download + getters  bitrate_selection/simulators/simulator.py:48-108
//   NetworkTrace.simulate_download         bitrate_selection/simulators/network.py:22-35
//   PlaybackBuffer.push_chunk              bitrate_selection/simulators/buffer.py:8-15
//   QoEModel.calculate_qoe                 bitrate_selection/utils/qoe.py:22-34
// The arithmetic is env_device.h's env_step_finish line for line (integer wave sum for the chunk size, trace walk and buffer in IEEE
// double with FMA contraction off, sequential float32 sums in tile order for the QoE), so a session stepped here with the versions
// mansy_allocate_tile_rates gives returns the same qoe_parts bits as mansy_env_step.
// The session record is the environment's (mansy_env_state_bytes / mansy_env_init / mansy_env_reset).  The history rings that
// describe actions (past_in, past_out, the one-hot) have no meaning without an action space: no ring is pushed and no observation is
// written.  ONE STATE BUFFER THEREFORE BELONGS EITHER TO A VECTOR ENVIRONMENT OR TO A SIMULATOR, NEVER TO BOTH.
// A step reads 2 x 1280 B of manifest rows, 256 B of versions, 64 B of viewport map and a few trace bins; it writes 2 x 256 B of
// tile rows, 64 B of viewport and ~50 B of scalars -- all of it as one coalesced 64-lane access per row.
// What-if (mansy_sim_lookahead / mansy_sim_peek_ahead, ExpertEnv.choose_action's pattern, bitrate_selection/envs/expert_env.py:358-422):
// K candidate plans of H chunks per session are downloaded virtually from the session's record, which is only read, with the same
// arithmetic, so a virtual step returns the bits the committed step would; the forward peek shows the table rows of the chunks a caller
// plans over.
// Making the plans (mansy_sim_allocate): one greedy per-tile allocation under a byte budget per (session, candidate, step), on the same
// table rows, from weights the caller brings or the predicted map.
// The planner loop (mansy_sim_drive): those three stages and the throughput estimate between them for D decisions per session in one
// launch, one workgroup per session, built from the device helpers the stand-alone kernels run.
// A client's belief (mansy_sim_lookahead_client / mansy_sim_drive_client): the what-if above is an oracle (the real trace, the
// ground-truth viewport of chunks not yet watched).  The same helpers, instantiated for a network model that divides the chunk size by
// a throughput estimate and pointed at the predicted map, score plans as a deployable client has to; the driving kernel then keeps a
// window of throughput samples per session and commits on the truth all the same.
// Budget schedules (mansy_sim_lookahead_schedules / mansy_sim_drive_schedules): a candidate takes one of F budget levels per step, all
// F^H sequences.  The allocation of a chunk depends on the chunk and its budget alone and everything tile-wide in a virtual step on
// that plan alone, so a workgroup makes F x H plans and step profiles with a wave each and walks the schedules with a LANE each, on
// the scalar half of the virtual step; the results are the bits of mansy_sim_allocate + mansy_sim_lookahead_client on the F^H x H plans.
#include "mansy_kernels.h"
#include "../../include/mansy_hip.h"

#pragma clang fp contract(off)

namespace {

#include "env_device.h"

// A record no session is open in: past its last chunk, or never reset since mansy_env_init (next_chunk == 0 there).
__device__ __forceinline__ bool session_closed(const mansy_env_tables& T, int next_chunk, int end_chunk) {
  return next_chunk > end_chunk || next_chunk <= T.startup_download;
}
// The chunks of a horizon of H the session still has: min(H, chunks left), 0 for a closed record.
__device__ __forceinline__ int steps_ahead(const mansy_env_tables& T, int next_chunk, int end_chunk, int H) {
  const int steps = session_closed(T, next_chunk, end_chunk) ? 0 : end_chunk - next_chunk + 1;
  return steps < H ? steps : H;
}
// Row addressing: element of (version 0, tile 0) of a chunk's manifest rows (five rows of 64 follow one another; the next chunk's
// begin NR * NTL further), and the cell of a chunk in the viewport tables (vp_acc: the cell, vp_gt / vp_pred: cell * NTL + tile).
__device__ __forceinline__ size_t manifest_row(const mansy_env_tables& T, int video, int chunk) {
  return ((size_t)video * T.n_chunk_max + chunk) * NR * NTL;
}
__device__ __forceinline__ size_t viewport_cell(const mansy_env_tables& T, int vp, int chunk) {
  return (size_t)vp * T.n_vpchunk_max + (chunk - T.vp_start[vp]);
}

__device__ __forceinline__ double seq_dsum64(float x) {      // ((..(0 + x0) + x1) ..) + x63 in float64, tile order (Python sum of a list)
  double s = 0.0;
#pragma unroll
  for (int t = 0; t < NTL; ++t) s = s + (double)__builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), t));
  return s;
}

// What a committed step hands back to the code around it (wave-uniform).
struct Committed { int chunk_size; double download_time; bool over; };

// One committed step by one wavefront (lane = tile) on the OPEN record s: Simulator.simulate_download, the QoE, the log and the step's
// outputs, then the next catalogue entry if the session ended and auto_reset asks for it.  ver: this lane's version (clamped here).
// The output pointers are the session's rows (tile rows of 64, scalars / qoe_parts rows of 4, one over flag; all but over nullable,
// launch-uniform).  The record is not stored here.
__device__ __forceinline__ Committed sim_commit(const mansy_env_tables& T, EnvRegs& s, int ver, int lane, float* tile_size, float* tile_quality,
                                                unsigned char* actual_viewport, double* scalars, float* qoe_parts, unsigned char* over_out,
                                                int auto_reset) {
  const int chunk = s.next_chunk;
  // ---- loads that depend on the state alone
  ver = ver < 0 ? 0 : ver > NR - 1 ? NR - 1 : ver;
  const size_t mrow = manifest_row(T, s.video, chunk);
  int size_r[NR]; float qual_r[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) { size_r[r] = T.size[mrow + r * NTL + lane]; qual_r[r] = T.quality[mrow + r * NTL + lane]; }
  const size_t vrow = viewport_cell(T, s.vp, chunk) * NTL;
  const unsigned char gt = T.vp_gt[vrow + lane];
  const float gv = (float)gt;
  const float* w = T.qoe_w + 3 * s.qoe;
  const float w0 = w[0], w1 = w[1], w2 = w[2];
  const double* bw = T.trace_bw + (size_t)s.trace * T.trace_len_max;
  const int tlen = T.trace_len[s.trace];
  double bwc = bw[s.cur_idx];
  const bool over_pre = chunk + 1 > s.end_chunk;
  const double acc_next = over_pre ? 0.0 : T.vp_acc[viewport_cell(T, s.vp, chunk + 1)];
  const float max_rate = (float)T.video_rates[NR - 1];
  // ---- Simulator.simulate_download
  int my_size = size_r[0]; float tq = qual_r[0];
#pragma unroll
  for (int r = 1; r < NR; ++r) { my_size = ver == r ? size_r[r] : my_size; tq = ver == r ? qual_r[r] : tq; }
  const int chunk_size = wave_isum(my_size);
  const double start = s.cur_time;
  double size = (double)chunk_size;
  while (size > 0) {
    const double fl = floor(s.cur_time + 1);
    const double remain = (fl - s.cur_time) * bwc;
    if (size >= remain) { s.cur_idx = s.cur_idx + 1 == tlen ? 0 : s.cur_idx + 1; bwc = bw[s.cur_idx]; s.cur_time = fl; size -= remain; }
    else { s.cur_time += size / bwc; size = 0; }
  }
  const double download_time = s.cur_time - start;
  double rebuf = 0.0;
  if (download_time > s.buf_size) { rebuf = download_time - s.buf_size; s.buf_size = (double)T.chunk_length; }
  else s.buf_size = s.buf_size - download_time + (double)T.chunk_length;
  s.next_chunk += 1;
  const bool over = s.next_chunk > s.end_chunk;
  // ---- QoEModel.calculate_qoe (sequential float32 sums in tile order)
  const ViewportSums vs = viewport_sums(gv, tq);
  const float s_v = vs.s_v;
  float vq = vs.s_vq / s_v;
  const float s_var = var_sum(vs, gv, tq, vq);
  const float intra = (s_var / s_v) / max_rate;
  vq = vq / max_rate;
  const float inter = s.has_prev ? fabsf(vq - s.prev_vq) : 0.f;
  s.prev_vq = vq; s.has_prev = 1;
  const float qoe1 = vq, qoe3 = intra + inter;
  const float qoe = w0 * qoe1 - w1 * (float)rebuf - w2 * qoe3;
  s.log_qoe += (double)qoe; s.log_qoe1 += (double)qoe1; s.log_qoe2 += rebuf; s.log_qoe3 += (double)qoe3; s.log_n += 1;
  s.buffer0 = (float)s.buf_size;
  if (!over) s.last_chunk_accuracy = acc_next;
  // ---- outputs
  if (tile_size) tile_size[lane] = (float)my_size;
  if (tile_quality) tile_quality[lane] = tq;
  if (actual_viewport) actual_viewport[lane] = gt;
  if (scalars) {                             // (a launch-uniform branch: the 64-term double chain is skipped when nobody asks)
    const double chunk_quality = seq_dsum64(tq);
    if (lane == 0) { scalars[0] = (double)chunk_size; scalars[1] = chunk_quality; scalars[2] = download_time; scalars[3] = rebuf; }
  }
  if (lane == 0) {
    if (qoe_parts) { qoe_parts[0] = qoe; qoe_parts[1] = qoe1; qoe_parts[2] = (float)rebuf; qoe_parts[3] = qoe3; }
    *over_out = over ? 1 : 0;
  }
  if (over && auto_reset) do_reset(T, s);    // the session opens its next catalogue entry, as the vector environment does
  Committed c;
  c.chunk_size = chunk_size; c.download_time = download_time; c.over = over;
  return c;
}

__global__ __launch_bounds__(256) void sim_download_kernel(mansy_env_tables T, EnvState* st, int n, const int* __restrict__ tile_rates,
                                                           float* tile_size, float* tile_quality, unsigned char* actual_viewport,
                                                           double* scalars, float* qoe_parts, unsigned char* over_out, int auto_reset) {
  const int e = __builtin_amdgcn_readfirstlane((blockIdx.x * 256 + threadIdx.x) >> 6), lane = threadIdx.x & 63;   // wave-uniform
  if (e >= n) return;
  const size_t row = (size_t)e * NTL + lane;
  EnvRegs s;
  load_state(s, st[e], lane);
  if (session_closed(T, s.next_chunk, s.end_chunk)) {
    if (!auto_reset) {                       // nothing to download: zeros, before any table is touched; the record stays as it is
      if (tile_size) tile_size[row] = 0.f;
      if (tile_quality) tile_quality[row] = 0.f;
      if (actual_viewport) actual_viewport[row] = 0;
      if (lane < 4) {
        if (scalars) scalars[4 * e + lane] = 0.0;
        if (qoe_parts) qoe_parts[4 * e + lane] = 0.f;
      }
      if (lane == 0) over_out[e] = 1;
      return;
    }
    do_reset(T, s);
  }
  const size_t tiles = (size_t)e * NTL;
  sim_commit(T, s, tile_rates[row], lane, tile_size ? tile_size + tiles : nullptr, tile_quality ? tile_quality + tiles : nullptr,
             actual_viewport ? actual_viewport + tiles : nullptr, scalars ? scalars + 4 * (size_t)e : nullptr,
             qoe_parts ? qoe_parts + 4 * (size_t)e : nullptr, over_out + e, auto_reset);
  store_state(st[e], s, lane);
}

__global__ __launch_bounds__(256) void sim_peek_kernel(mansy_env_tables T, const EnvState* __restrict__ st, int n, int* next_chunk, double* buffer,
                                                       float* size, float* quality, unsigned char* gt, unsigned char* pred, double* acc) {
  const int e = __builtin_amdgcn_readfirstlane((blockIdx.x * 256 + threadIdx.x) >> 6), lane = threadIdx.x & 63;   // wave-uniform
  if (e >= n) return;
  const EnvState& s = st[e];
  const int chunk = s.next_chunk, video = s.video, vp = s.vp;
  const bool closed = session_closed(T, chunk, s.end_chunk);
  const size_t row = (size_t)e * NTL + lane;
  if (lane == 0) {
    if (next_chunk) next_chunk[e] = closed ? 0 : chunk;
    if (buffer) buffer[e] = closed ? 0.0 : s.buf_size;
    if (acc) acc[e] = closed ? 0.0 : s.last_chunk_accuracy;
  }
  if (closed) {                              // no table row belongs to a closed session: zeros without a load
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      if (size) size[((size_t)e * NR + r) * NTL + lane] = 0.f;
      if (quality) quality[((size_t)e * NR + r) * NTL + lane] = 0.f;
    }
    if (gt) gt[row] = 0;
    if (pred) pred[row] = 0;
    return;
  }
  const size_t mrow = manifest_row(T, video, chunk);
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    if (size) size[((size_t)e * NR + r) * NTL + lane] = (float)T.size[mrow + r * NTL + lane];
    if (quality) quality[((size_t)e * NR + r) * NTL + lane] = T.quality[mrow + r * NTL + lane];
  }
  const size_t vrow = viewport_cell(T, vp, chunk) * NTL;
  if (gt) gt[row] = T.vp_gt[vrow + lane];
  if (pred) pred[row] = T.vp_pred[vrow + lane];
}

// ---- what-if: candidate plans downloaded virtually from a session's record, which is only read (expert_env.py:358-422 for arbitrary
// tile versions).  LookState is the part of the record a download moves and a QoE term reads; it lives in registers of the wave
// that walks one candidate and is dropped at the end.
struct LookState { double cur_time, buf_size, bwc; int cur_idx, has_prev; float prev_vq, sum; };
struct LookConst { const double* bw; int tlen; float w0, w1, w2, max_rate; double chunk_length, rate; };
// How a virtual download takes its time: the walk over the session's real trace from where the record stands (the oracle's), or one
// division by the bytes/s the caller believes in (a client's; the trace position of the record is then not read).
constexpr int NET_TRACE = MANSY_SIM_NET_TRACE, NET_ESTIMATE = MANSY_SIM_NET_ESTIMATE;

// One virtual step is sim_download_kernel's arithmetic from "Simulator.simulate_download" to the QoE, line for line, in a tile-wide part
// and a scalar part.  The tile-wide part, by one wavefront (lane = tile) on the tile's size / quality of the planned version and the
// chunk's viewport map gv (ground truth or prediction): what the step has of the chunk and its plan alone, the same in every lane --
// the integer chunk size (wave_isum), and the viewport quality (qoe1) with the intra-chunk variance (look_quality).
struct StepProfile { int chunk_size; float vq, intra; };
__device__ __forceinline__ void look_quality(StepProfile& p, float tq, float gv, float max_rate) {
  const ViewportSums vs = viewport_sums(gv, tq);
  const float s_v = vs.s_v;
  const float vq = vs.s_vq / s_v;
  const float s_var = var_sum(vs, gv, tq, vq);
  p.intra = (s_var / s_v) / max_rate;
  p.vq = vq / max_rate;
}
__device__ __forceinline__ StepProfile look_profile(int my_size, float tq, float gv, float max_rate) {
  StepProfile p;
  p.chunk_size = wave_isum(my_size);
  look_quality(p, tq, gv, max_rate);
  return p;
}
// The scalar part, on the state the candidate carries from step to step: the download (the walk over the trace, or with NET_ESTIMATE
// download_time = chunk_size / c.rate in plain IEEE double, whatever c.rate holds) with the buffer rule (look_download), then
// |vq - prev_vq|, the QoE and the float32 running total (look_score).  Nothing here looks at a tile, so a single lane may run it on a
// profile another wave made (the schedule search).
struct StepScalars { double download_time, rebuf; float qoe, qoe3; };
template <int NET>
__device__ __forceinline__ void look_download(LookState& s, const LookConst& c, int chunk_size, StepScalars& r) {
  if constexpr (NET == NET_TRACE) {
    const double start = s.cur_time;
    double size = (double)chunk_size;
    while (size > 0) {
      const double fl = floor(s.cur_time + 1);
      const double remain = (fl - s.cur_time) * s.bwc;
      if (size >= remain) { s.cur_idx = s.cur_idx + 1 == c.tlen ? 0 : s.cur_idx + 1; s.bwc = c.bw[s.cur_idx]; s.cur_time = fl; size -= remain; }
      else { s.cur_time += size / s.bwc; size = 0; }
    }
    r.download_time = s.cur_time - start;
  } else {
    r.download_time = (double)chunk_size / c.rate;
  }
  r.rebuf = 0.0;
  if (r.download_time > s.buf_size) { r.rebuf = r.download_time - s.buf_size; s.buf_size = c.chunk_length; }
  else s.buf_size = s.buf_size - r.download_time + c.chunk_length;
}
__device__ __forceinline__ void look_score(LookState& s, const LookConst& c, const StepProfile& p, StepScalars& r) {
  const float inter = s.has_prev ? fabsf(p.vq - s.prev_vq) : 0.f;
  s.prev_vq = p.vq; s.has_prev = 1;
  r.qoe3 = p.intra + inter;
  r.qoe = c.w0 * p.vq - c.w1 * (float)r.rebuf - c.w2 * r.qoe3;
  s.sum = s.sum + r.qoe;                     // ((0 + qoe_0) + qoe_1) + .. : plan_step's ps.sum (env.hip)
}
template <int NET>
__device__ __forceinline__ void look_scalars(LookState& s, const LookConst& c, const StepProfile& p) {
  StepScalars r;
  look_download<NET>(s, c, p.chunk_size, r);
  look_score(s, c, p, r);
}
// One virtual step by one wavefront: the two parts, their halves in the order of the committed step (size, download, quality, score).
// qoe_row / sc_row: this step's four-value output rows (nullable, launch-uniform).
template <int NET>
__device__ __forceinline__ void look_step(LookState& s, const LookConst& c, int my_size, float tq, float gv, int lane, float* qoe_row,
                                          double* sc_row) {
  StepProfile p;
  StepScalars r;
  p.chunk_size = wave_isum(my_size);
  look_download<NET>(s, c, p.chunk_size, r);
  look_quality(p, tq, gv, c.max_rate);
  look_score(s, c, p, r);
  if (sc_row) {
    const double chunk_quality = seq_dsum64(tq);
    if (lane == 0) { sc_row[0] = (double)p.chunk_size; sc_row[1] = chunk_quality; sc_row[2] = r.download_time; sc_row[3] = r.rebuf; }
  }
  if (qoe_row && lane == 0) { qoe_row[0] = r.qoe; qoe_row[1] = p.vq; qoe_row[2] = (float)r.rebuf; qoe_row[3] = r.qoe3; }
}

struct LookTile { int size; float quality, gv; };
// The table values lane's tile has in virtual step t: the planned version's size and quality (a 64-lane gather over the chunk's five
// 256 B rows) and the viewport map vmap (T.vp_gt or T.vp_pred, launch-uniform).  mrow / vrow: this lane's element of the session's
// NEXT chunk.
__device__ __forceinline__ LookTile look_load(const mansy_env_tables& T, const unsigned char* __restrict__ vmap, int ver, size_t mrow, size_t vrow,
                                              int t) {
  ver = ver < 0 ? 0 : ver > NR - 1 ? NR - 1 : ver;
  const size_t m = mrow + ((size_t)t * NR + ver) * NTL;
  LookTile r;
  r.size = T.size[m]; r.quality = T.quality[m]; r.gv = (float)vmap[vrow + (size_t)t * NTL];
  return r;
}

// The fields of a record that planning reads: where the session stands and what a virtual download starts from.  The kernels that
// only read a record take them from HBM; the driving kernel keeps them in LDS between the steps it commits.
struct SessionView { int video, vp, trace, qoe, next_chunk, end_chunk, cur_idx, has_prev; double cur_time, buf_size; float prev_vq; };
template <typename Rec>
__device__ __forceinline__ SessionView view_of(const Rec& r) {
  SessionView v;
  v.video = r.video; v.vp = r.vp; v.trace = r.trace; v.qoe = r.qoe; v.next_chunk = r.next_chunk; v.end_chunk = r.end_chunk;
  v.cur_idx = r.cur_idx; v.has_prev = r.has_prev; v.cur_time = r.cur_time; v.buf_size = r.buf_size; v.prev_vq = r.prev_vq;
  return v;
}

// Where lane's versions of a plan come from: int32 rows of 64 in the caller's memory, or the byte rows the driving kernel keeps in LDS.
struct PlanRows { const int* p; __device__ __forceinline__ int operator()(int t) const { return p[(size_t)t * NTL]; } };
struct PlanBytes { const unsigned char* p; __device__ __forceinline__ int operator()(int t) const { return p[t * NTL]; } };

// What the virtual steps of a session share (the trace, the QoE weights, rate: the bytes/s of NET_ESTIMATE) and the state a candidate
// starts from: where the record stands, an empty total.
template <int NET>
__device__ __forceinline__ LookConst look_const(const mansy_env_tables& T, const SessionView& r, double rate) {
  const float* w = T.qoe_w + 3 * r.qoe;
  LookConst c;
  if constexpr (NET == NET_TRACE) { c.bw = T.trace_bw + (size_t)r.trace * T.trace_len_max; c.tlen = T.trace_len[r.trace]; }
  else { c.bw = nullptr; c.tlen = 0; }
  c.rate = rate;
  c.w0 = w[0]; c.w1 = w[1]; c.w2 = w[2]; c.max_rate = (float)T.video_rates[NR - 1]; c.chunk_length = (double)T.chunk_length;
  return c;
}
template <int NET>
__device__ __forceinline__ LookState look_start(const SessionView& r, const LookConst& c) {
  LookState s;
  s.cur_time = r.cur_time; s.buf_size = r.buf_size; s.cur_idx = r.cur_idx; s.has_prev = r.has_prev; s.prev_vq = r.prev_vq; s.sum = 0.f;
  s.bwc = NET == NET_TRACE ? c.bw[s.cur_idx] : 0.0;
  return s;
}

// One candidate walked by one wavefront (lane = tile) over steps >= 1 chunks from where the session stands; returns the float32 total.
// The loads of step t + 1 depend on t alone, not on the download of step t, so they are issued before that step's dependent chain
// (trace walk, sequential sums) instead of behind it.  qoe_parts / scalars: the candidate's [H,4] rows (nullable, launch-uniform).
// NET / rate: look_step's network model and, for NET_ESTIMATE, the session's bytes/s; vmap: the viewport table the steps are scored on.
template <int NET, typename Plan>
__device__ __forceinline__ float look_walk(const mansy_env_tables& T, const SessionView& r, int steps, const Plan& plan, int lane, double rate,
                                           const unsigned char* __restrict__ vmap, float* qoe_parts, double* scalars) {
  const int chunk = r.next_chunk;
  const LookConst c = look_const<NET>(T, r, rate);
  LookState s = look_start<NET>(r, c);
  const size_t mrow = manifest_row(T, r.video, chunk) + lane;
  const size_t vrow = viewport_cell(T, r.vp, chunk) * NTL + lane;
  LookTile next = look_load(T, vmap, plan(0), mrow, vrow, 0);
  for (int t = 0; t < steps; ++t) {
    const LookTile cur = next;
    if (t + 1 < steps) next = look_load(T, vmap, plan(t + 1), mrow, vrow, t + 1);
    look_step<NET>(s, c, cur.size, cur.quality, cur.gv, lane, qoe_parts ? qoe_parts + t * 4 : nullptr, scalars ? scalars + t * 4 : nullptr);
  }
  return s.sum;
}

// One wavefront per (session, candidate), lane = tile, looping over the horizon.  The K candidates of a session read the same table
// rows; they meet in the caches.  A form that staged the rows of the horizon in LDS once per (session, 16 candidates) was measured and
// was not faster beyond the run-to-run spread, so this plain form is the only one.
// NET_TRACE with vmap = T.vp_gt is mansy_sim_lookahead; throughput (f64 [n]) is read by NET_ESTIMATE alone.
template <int NET>
__global__ __launch_bounds__(256) void sim_lookahead_kernel(mansy_env_tables T, const EnvState* __restrict__ st, int n, const int* __restrict__ plans,
                                                            int K, int H, const double* __restrict__ throughput,
                                                            const unsigned char* __restrict__ vmap, float* qoe_parts, double* scalars, float* total,
                                                            int* steps_out) {
  const long long wave = ((long long)blockIdx.x * 256 + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (wave >= (long long)n * K) return;
  const int e = __builtin_amdgcn_readfirstlane((int)(wave / K)), k = __builtin_amdgcn_readfirstlane((int)(wave % K));   // wave-uniform
  const EnvState& r = st[e];
  const int steps = steps_ahead(T, r.next_chunk, r.end_chunk, H);
  const size_t cand = (size_t)e * K + k;
  if (k == 0 && lane == 0) steps_out[e] = steps;
  for (int t = steps; t < H; ++t) {          // steps that are not simulated: zeros, and no table row is touched for them
    if (lane < 4) {
      if (qoe_parts) qoe_parts[(cand * H + t) * 4 + lane] = 0.f;
      if (scalars) scalars[(cand * H + t) * 4 + lane] = 0.0;
    }
  }
  if (steps == 0) { if (lane == 0) total[cand] = 0.f; return; }
  const PlanRows plan = {plans + cand * H * NTL + lane};
  const double rate = NET == NET_ESTIMATE ? throughput[e] : 0.0;
  const float sum = look_walk<NET>(T, view_of(r), steps, plan, lane, rate, vmap, qoe_parts ? qoe_parts + cand * H * 4 : nullptr,
                                   scalars ? scalars + cand * H * 4 : nullptr);
  if (lane == 0) total[cand] = sum;
}

// (total, candidate) as one order-preserving 64-bit key: the larger total wins, then the smaller index; 0 for a NaN, which therefore
// never beats anything.  The reference keeps the first plan with the strictly largest sum (`if best < qoe_sum`, expert_env.py:411).
__device__ __forceinline__ unsigned long long total_key(float v, unsigned idx) {
  if (v != v) return 0ull;
  unsigned u = __float_as_uint(v == 0.f ? 0.f : v);                // -0.0 == 0.0 in that comparison
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)u << 32) | (unsigned long long)(0xFFFFFFFFu - idx);
}

// One wavefront scans the K totals of a session: the index of the best one, in every lane.  Every total a NaN (all keys 0): candidate 0.
__device__ __forceinline__ int best_of(const float* row, int K, int lane) {
  unsigned long long key = 0ull;
  for (int k = lane; k < K; k += NTL) {
    const unsigned long long other = total_key(row[k], (unsigned)k);
    key = other > key ? other : key;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(key, o, 64);
    key = other > key ? other : key;
  }
  return key == 0ull ? 0 : (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
}

__global__ __launch_bounds__(256) void sim_best_kernel(const float* __restrict__ total, int n, int K, int* best, float* best_total) {
  const int e = __builtin_amdgcn_readfirstlane((blockIdx.x * 256 + threadIdx.x) >> 6), lane = threadIdx.x & 63;   // wave-uniform
  if (e >= n) return;
  const float* row = total + (size_t)e * K;
  const int idx = best_of(row, K, lane);
  if (lane == 0) {
    if (best) best[e] = idx;
    if (best_total) best_total[e] = row[idx];
  }
}

__global__ __launch_bounds__(256) void sim_peek_ahead_kernel(mansy_env_tables T, const EnvState* __restrict__ st, int n, int ahead, float* size,
                                                             float* quality, unsigned char* gt, unsigned char* pred, double* acc,
                                                             unsigned char* valid) {
  const int e = __builtin_amdgcn_readfirstlane((blockIdx.x * 256 + threadIdx.x) >> 6), lane = threadIdx.x & 63;   // wave-uniform
  if (e >= n) return;
  const EnvState& s = st[e];
  const int chunk = s.next_chunk + ahead, video = s.video, vp = s.vp;
  const bool ok = !session_closed(T, s.next_chunk, s.end_chunk) && chunk <= s.end_chunk;
  const size_t row = (size_t)e * NTL + lane;
  if (lane == 0) valid[e] = ok ? 1 : 0;
  if (!ok) {                                 // no table row belongs to a chunk past the session's end: zeros without a load
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      if (size) size[((size_t)e * NR + r) * NTL + lane] = 0.f;
      if (quality) quality[((size_t)e * NR + r) * NTL + lane] = 0.f;
    }
    if (gt) gt[row] = 0;
    if (pred) pred[row] = 0;
    if (acc && lane == 0) acc[e] = 0.0;
    return;
  }
  const size_t mrow = manifest_row(T, video, chunk);
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    if (size) size[((size_t)e * NR + r) * NTL + lane] = (float)T.size[mrow + r * NTL + lane];
    if (quality) quality[((size_t)e * NR + r) * NTL + lane] = T.quality[mrow + r * NTL + lane];
  }
  const size_t vcell = viewport_cell(T, vp, chunk);
  if (gt) gt[row] = T.vp_gt[vcell * NTL + lane];
  if (pred) pred[row] = T.vp_pred[vcell * NTL + lane];
  // the accuracy a session shows when it reaches that chunk (do_reset / the step's acc_next read this table cell); the record's own copy
  // for ahead == 0, as mansy_sim_peek shows it
  if (acc && lane == 0) acc[e] = ahead == 0 ? s.last_chunk_accuracy : T.vp_acc[vcell];
}

// ---- budgeted per-tile allocation: the plans a look-ahead scores, made from a byte budget and a weight per tile.  One (session,
// candidate, step) is a 64-item multiple-choice knapsack solved greedily: every tile starts at version 0 and, round by round, the
// upgrade (one version up on one tile) with the largest gain per byte that still fits the budget is applied, gain = weight x quality
// difference in float64, the lowest tile among equal ratios, an upgrade that costs no bytes before all that cost some (mansy_hip.h has
// the definition to the bit).
// The largest float64 of the wave, in every lane.  No NaN comes in here, so the order of the comparisons does not show in the result:
// DPP row rotations inside each row of 16 lanes, then the four rows by readlane (mansy_common.h's wave_max for two registers; a
// __shfl_xor is an LDS-pipe round trip per register and step, and a round of the allocator waits for this maximum).
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)u, CTRL, 0xf, 0xf, false);
  const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(u >> 32), CTRL, 0xf, 0xf, false);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ double lane_f64(double v, int lane) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, lane), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), lane);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ double dmax2(double a, double b) { return b > a ? b : a; }
__device__ __forceinline__ double wave_dmax(double v) {
  v = dmax2(v, dpp_f64<0x128>(v)); v = dmax2(v, dpp_f64<0x124>(v)); v = dmax2(v, dpp_f64<0x122>(v)); v = dmax2(v, dpp_f64<0x121>(v));
  return dmax2(dmax2(lane_f64(v, 0), lane_f64(v, 16)), dmax2(lane_f64(v, 32), lane_f64(v, 48)));
}

// One allocation by one wavefront, lane = tile.  The lane keeps what its tile's four upgrades need in registers: they do not depend on
// the round, so their byte differences, the signs of their gains and their ratios (the only float64 divisions) are formed once, from
// the five sizes and qualities of the tile in chunk `chunk` of (video, vp) and the weights row w_row (64 floats) or, for w_row ==
// nullptr, the chunk's predicted map.  base: the integer sum of the 64 version-0 sizes (wave-uniform).
struct AllocTile { int ds_u[NR - 1]; double ratio_u[NR - 1]; bool gain_u[NR - 1]; int base; };
__device__ __forceinline__ AllocTile alloc_tile(const mansy_env_tables& T, int video, int vp, int chunk, const float* __restrict__ w_row, int lane) {
  const size_t mrow = manifest_row(T, video, chunk) + lane;
  int size_r[NR]; float qual_r[NR];
#pragma unroll
  for (int v = 0; v < NR; ++v) { size_r[v] = T.size[mrow + v * NTL]; qual_r[v] = T.quality[mrow + v * NTL]; }
  const float w = w_row ? w_row[lane] : (float)T.vp_pred[viewport_cell(T, vp, chunk) * NTL + lane];
  AllocTile a;
#pragma unroll
  for (int v = 0; v < NR - 1; ++v) {
    const float dq = qual_r[v + 1] - qual_r[v];
    const double gain = (double)w * (double)dq;
    a.ds_u[v] = size_r[v + 1] - size_r[v];
    a.gain_u[v] = gain > 0.0;                 // false for a NaN
    a.ratio_u[v] = a.ds_u[v] <= 0 ? __builtin_huge_val() : gain / (double)a.ds_u[v];
  }
  a.base = wave_isum(size_r[0]);
  return a;
}
// The rounds of an allocation from round `round` on, where the lane's tile stands at version ver and the plan holds `total` bytes (0,
// 0 and a.base: a whole allocation).  A round selects the tile's next upgrade by its version, then: 64-lane maximum of the candidates'
// ratios (-1 stands for "not a candidate": a candidate's ratio is >= 0), ballot of the candidates that hold it, lowest set bit wins,
// and the winner's byte difference reaches the wave-uniform total by readlane.  An empty ballot ends the loop, after 256 rounds at the
// latest.  rec_win / rec_total (nullable): the winner and the total after every round that upgraded, for alloc_resume; returns the
// number of those rounds, counted from 0.
__device__ __forceinline__ int alloc_rounds(const AllocTile& a, double budget, int lane, int round, int& ver, int& total, unsigned char* rec_win,
                                            int* rec_total) {
  for (; round < NTL * (NR - 1); ++round) {
    int ds = 0; double ratio = -1.0; bool gains = false;         // ver == 4: no upgrade is left
#pragma unroll
    for (int v = 0; v < NR - 1; ++v) if (ver == v) { ds = a.ds_u[v]; ratio = a.ratio_u[v]; gains = a.gain_u[v]; }
    const bool cand = gains && (double)(total + ds) <= budget;   // false for a NaN budget
    const double key = cand ? ratio : -1.0;
    const double top = wave_dmax(key);
    const unsigned long long winners = __ballot(cand && key == top);
    if (winners == 0ull) break;
    const int win = __builtin_ctzll(winners);
    total += __builtin_amdgcn_readlane(ds, win);
    ver += lane == win ? 1 : 0;
    if (rec_win && lane == 0) { rec_win[round] = (unsigned char)win; rec_total[round] = total; }
  }
  return round;
}
// Where the allocation under `budget` stands after the rounds it shares with a recorded allocation of the same tiles under `lead`.
// While the recorded winner of a round also fits `budget` it is this allocation's winner too: with budget <= lead this allocation's
// candidates are a subset of the recorded one's (the fit test is the only place the budget enters), the recorded winner is the lowest
// tile among the largest ratios of the superset, so where it belongs to the subset it is that of the subset as well, and the state
// after the round is the same.  The first recorded round whose total does not fit ends the shared part (a NaN budget: round 0); the
// rounds go on from there by alloc_rounds.  Not budget <= lead (a NaN on either side included): nothing is shared.  Returns the round
// to go on from and sets the lane's version and the total there.
__device__ __forceinline__ int alloc_resume(const AllocTile& a, double budget, double lead, int lane, const unsigned char* rec_win, const int* rec_total,
                                            int rounds, int& ver, int& total) {
  int shared = 0;
  if (__ballot(budget <= lead) != 0ull) {
    shared = rounds;
    for (int r0 = 0; r0 < rounds; r0 += NTL) {
      const int r = r0 + lane;
      const unsigned long long fails = __ballot(r < rounds && !((double)rec_total[r < rounds ? r : 0] <= budget));
      if (fails != 0ull) { shared = r0 + __builtin_ctzll(fails); break; }
    }
  }
  ver = 0;
  for (int r = 0; r < shared; ++r) ver += rec_win[r] == lane ? 1 : 0;
  total = shared > 0 ? rec_total[shared - 1] : a.base;
  return shared;
}

// One wavefront per (session, candidate, step).
__global__ __launch_bounds__(256) void sim_allocate_kernel(mansy_env_tables T, const EnvState* __restrict__ st, int n, const double* __restrict__ budgets,
                                                           const float* __restrict__ weights, int K, int H, int* plans, int* plan_bytes,
                                                           int* steps_out) {
  const long long wave = ((long long)blockIdx.x * 256 + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (wave >= (long long)n * K * H) return;
  const int KH = K * H;
  const int e = __builtin_amdgcn_readfirstlane((int)(wave / KH)), kt = __builtin_amdgcn_readfirstlane((int)(wave % KH));   // wave-uniform
  const int t = kt % H;
  const EnvState& r = st[e];
  const int chunk = r.next_chunk;
  const int steps = steps_ahead(T, chunk, r.end_chunk, H);
  if (kt == 0 && lane == 0) steps_out[e] = steps;
  const size_t row = (size_t)wave;            // (e * K + k) * H + t
  if (t >= steps) {                           // a chunk past the session's end: zeros, and no table row is touched for it
    plans[row * NTL + lane] = 0;
    if (plan_bytes && lane == 0) plan_bytes[row] = 0;
    return;
  }
  const AllocTile a = alloc_tile(T, r.video, r.vp, chunk + t, weights ? weights + ((size_t)e * H + t) * NTL : nullptr, lane);
  int ver = 0, total = a.base;
  alloc_rounds(a, budgets[row], lane, 0, ver, total, nullptr, nullptr);
  plans[row * NTL + lane] = ver;
  if (plan_bytes && lane == 0) plan_bytes[row] = total;
}

// ---- the planner loop in one launch: D decisions of allocate -> look-ahead -> commit -> throughput estimate per session, with the
// plans, the totals and the record kept on chip (mansy_hip.h has the definition; every stage is the helper the stand-alone kernel of
// that stage runs, so a decision returns the bits the three launches and the torch between them would).
// One workgroup of WAVES wavefronts per session (16 or 4, chosen by the number of sessions), lane = tile.  LDS: K float32 totals, then
// the K x H plans as bytes (version 0..4 of a tile), [k][t][tile] -- 32.25 KB at K = 64, H = 8 -- and the session's record with the
// throughput estimate and the recorded rounds of the leading allocations (10 KB).  A decision:
//   one wave per chunk makes the allocation under the largest budget and records its rounds      | barrier
//   the waves share out the other allocations, each resumed where it leaves the recorded rounds  | barrier
//   (rows t >= steps are never made: nothing reads them)
//   the waves share out the K walks                                                              | barrier
//   wave 0 picks the best and commits its first step on the record in LDS (registers in between) | barrier
// EVERY WAVE REACHES EVERY BARRIER: D is a kernel argument, steps comes from the one record all waves read after the same barrier, and
// no barrier stands inside a condition.  The record comes from HBM once and goes back once, after the last decision, if a step moved it.
struct DriveShared {
  EnvState rec; double throughput;
  int rounds[MANSY_SIM_MAX_HORIZON], rec_total[MANSY_SIM_MAX_HORIZON][NTL * (NR - 1)];   // the leading allocation of every chunk, round by round
  unsigned char rec_win[MANSY_SIM_MAX_HORIZON][NTL * (NR - 1)];
};
constexpr int DRIVE_WIDE_SESSIONS = 256;   // up to one session per CU of an MI355X: the wide workgroup
// The client's loop (mansy_sim_drive_client) keeps the session's throughput samples beside the record: the newest at index 7.
struct DriveSharedClient : DriveShared { double history[MANSY_SIM_EST_MAX_WINDOW]; int count; };
// The schedule search (mansy_sim_lookahead_schedules / mansy_sim_drive_schedules) keeps what the F^H schedules are made of: the F x H
// plans as bytes, [f][t][tile], and the step profile of every one of them.
constexpr int SCHED_STEPS = MANSY_SIM_SCHED_MAX_LEVELS * MANSY_SIM_MAX_HORIZON;
struct SchedShared : DriveSharedClient {
  unsigned char plans[SCHED_STEPS * NTL];
  int chunk_size[SCHED_STEPS]; float vq[SCHED_STEPS], intra[SCHED_STEPS];
};
struct DriveOracle { using Shared = DriveShared; static constexpr bool client = false, schedules = false; };
struct DriveClient { using Shared = DriveSharedClient; static constexpr bool client = true, schedules = false; };
struct DriveSchedules { using Shared = SchedShared; static constexpr bool client = true, schedules = true; };

// The estimator of mansy_sim_drive_client after a committed step with download_time > 0, by ONE lane on the slots in LDS: the slots
// shift down by one, the sample goes in at the top, and the estimate is the harmonic mean of the newest min(window, count) samples,
// summed oldest first (the sample itself for one).  Returns the estimate.
__device__ __forceinline__ double estimate_push(double* history, int& count, double sample, int window) {
  constexpr int W = MANSY_SIM_EST_MAX_WINDOW;
  for (int j = 0; j < W - 1; ++j) history[j] = history[j + 1];
  history[W - 1] = sample;
  count = count + 1 < W ? count + 1 : W;
  const int m = window < count ? window : count;
  if (m == 1) return sample;
  double sum = 1.0 / history[W - m];
  for (int j = W - m + 1; j < W; ++j) sum = sum + 1.0 / history[j];
  return (double)m / sum;
}

// The allocations of one decision by the WAVES wavefronts of a session's workgroup: plans[(k * H + t) * 64 + tile] for K budgets
// per_chunk * fractions[k] over the `steps` chunks the session has ahead.  The candidate with the largest budget leads: one wave per
// chunk records its rounds, the others go on from the rounds they share.  TWO BARRIERS, reached by every wave: one after the leading
// allocations, one after the rest.
template <int WAVES>
__device__ __forceinline__ void drive_allocate(const mansy_env_tables& T, const SessionView& v, int steps, double per_chunk,
                                               const double* __restrict__ fractions, int K, int H, unsigned char* plans, DriveShared& sh, int wave,
                                               int lane) {
  int lead_k = 0;
  double lead = per_chunk * fractions[0];
  for (int k = 1; k < K; ++k) {
    const double budget = per_chunk * fractions[k];
    if (__ballot(budget > lead) != 0ull) { lead = budget; lead_k = k; }
  }
  for (int t = wave; t < steps; t += WAVES) {
    const AllocTile a = alloc_tile(T, v.video, v.vp, v.next_chunk + t, nullptr, lane);
    int ver = 0, total = a.base;
    const int rounds = alloc_rounds(a, lead, lane, 0, ver, total, sh.rec_win[t], sh.rec_total[t]);
    if (lane == 0) sh.rounds[t] = rounds;
    plans[(lead_k * H + t) * NTL + lane] = (unsigned char)ver;
  }
  __syncthreads();
  const int KS = K * steps;
  for (int kt = wave; kt < KS; kt += WAVES) {
    const int k = kt / steps, t = kt - k * steps;
    if (k == lead_k) continue;
    const double budget = per_chunk * fractions[k];
    const AllocTile a = alloc_tile(T, v.video, v.vp, v.next_chunk + t, nullptr, lane);
    int ver, total;
    const int round = alloc_resume(a, budget, lead, lane, sh.rec_win[t], sh.rec_total[t], __builtin_amdgcn_readfirstlane(sh.rounds[t]), ver, total);
    alloc_rounds(a, budget, lane, round, ver, total, nullptr, nullptr);
    plans[(k * H + t) * NTL + lane] = (unsigned char)ver;
  }
  __syncthreads();
}

// The F^steps schedule prefixes of a session walked with a lane per prefix on the step profiles in LDS: prefix p uses at step t the
// level (p / F^(steps-1-t)) % F, and its float32 total goes to totals[p].  The lanes of a wave diverge in the trace walk's loop.
template <int NET>
__device__ __forceinline__ void sched_walk(const mansy_env_tables& T, const SessionView& v, int steps, int P, int F, int H, double rate,
                                           const SchedShared& sh, float* totals, int thread, int threads) {
  if (P == 0) return;                         // a closed record (the same in every thread; no barrier in here)
  const LookConst c = look_const<NET>(T, v, rate);
  const LookState start = look_start<NET>(v, c);
  for (int p = thread; p < P; p += threads) {
    LookState s = start;
    int place = P / F;                        // F^(steps-1-t)
    for (int t = 0; t < steps; ++t) {
      const int ft = (p / place) % F * H + t;
      place = place / F;
      StepProfile q;
      q.chunk_size = sh.chunk_size[ft]; q.vq = sh.vq[ft]; q.intra = sh.intra[ft];
      look_scalars<NET>(s, c, q);
    }
    totals[p] = s.sum;
  }
}

// The schedule search of one session by its workgroup at the estimate thr: the F x steps allocations under thr x chunk_length x
// levels[f] into sh.plans (drive_allocate), one wave per (f, t) for the step profile of that plan on vmap, then the walks.  Returns
// P = F^steps, the number of prefixes that differ (0 for a closed record), with totals[0 .. P) filled: the F^H schedules that share a
// prefix share its total, and the first of them is F^(H-steps) x the prefix.  FOUR BARRIERS, reached by every wave, the last one
// behind the walks.
template <int WAVES>
__device__ __forceinline__ int sched_search(const mansy_env_tables& T, const SessionView& v, int steps, double thr, const double* __restrict__ levels,
                                            int F, int H, int network, const unsigned char* __restrict__ vmap, SchedShared& sh, float* totals,
                                            int wave, int lane) {
  drive_allocate<WAVES>(T, v, steps, thr * (double)T.chunk_length, levels, F, H, sh.plans, sh, wave, lane);
  const int FS = F * steps;
  for (int ft = wave; ft < FS; ft += WAVES) {
    const int f = ft / steps, t = ft - f * steps;
    const size_t mrow = manifest_row(T, v.video, v.next_chunk) + lane;
    const size_t vrow = viewport_cell(T, v.vp, v.next_chunk) * NTL + lane;
    const LookTile x = look_load(T, vmap, sh.plans[(f * H + t) * NTL + lane], mrow, vrow, t);
    const StepProfile p = look_profile(x.size, x.quality, x.gv, (float)T.video_rates[NR - 1]);
    if (lane == 0) { sh.chunk_size[f * H + t] = p.chunk_size; sh.vq[f * H + t] = p.vq; sh.intra[f * H + t] = p.intra; }
  }
  __syncthreads();
  int P = steps > 0 ? 1 : 0;
  for (int t = 0; t < steps; ++t) P *= F;
  const int thread = wave * NTL + lane;
  if (network == NET_ESTIMATE) sched_walk<NET_ESTIMATE>(T, v, steps, P, F, H, thr, sh, totals, thread, WAVES * NTL);   // (a kernel argument)
  else sched_walk<NET_TRACE>(T, v, steps, P, F, H, 0.0, sh, totals, thread, WAVES * NTL);
  __syncthreads();
  return P;
}

// One workgroup per session, as the driving kernel below; the record is only read.  totals: dynamic LDS, F^H floats.
template <int WAVES>
__global__ __launch_bounds__(WAVES * 64) void sim_lookahead_schedules_kernel(mansy_env_tables T, const EnvState* __restrict__ st,
                                                                             const double* __restrict__ levels, int F, int H, int K,
                                                                             const double* __restrict__ throughput, int network,
                                                                             const unsigned char* __restrict__ vmap, int* level_plans, int* level_bytes,
                                                                             float* total, int* steps_out, int* best, float* best_total) {
  extern __shared__ __align__(16) unsigned char sched_lds[];
  __shared__ SchedShared sh;
  float* totals = (float*)sched_lds;
  const int e = blockIdx.x, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  SessionView v = view_of(st[e]);             // the same values in every lane of the workgroup; the integers into scalar registers
  v.video = __builtin_amdgcn_readfirstlane(v.video); v.vp = __builtin_amdgcn_readfirstlane(v.vp);
  v.trace = __builtin_amdgcn_readfirstlane(v.trace); v.qoe = __builtin_amdgcn_readfirstlane(v.qoe);
  v.next_chunk = __builtin_amdgcn_readfirstlane(v.next_chunk); v.end_chunk = __builtin_amdgcn_readfirstlane(v.end_chunk);
  v.cur_idx = __builtin_amdgcn_readfirstlane(v.cur_idx); v.has_prev = __builtin_amdgcn_readfirstlane(v.has_prev);
  const int steps = steps_ahead(T, v.next_chunk, v.end_chunk, H);
  const int P = sched_search<WAVES>(T, v, steps, throughput[e], levels, F, H, network, vmap, sh, totals, wave, lane);
  const int leaves = P > 0 ? K / P : K;        // the schedules that share a prefix: F^(H-steps)
  if (wave == 0) {
    const int b = P > 0 ? best_of(totals, P, lane) : 0;
    if (lane == 0) {
      steps_out[e] = steps;
      if (best) best[e] = b * leaves;
      if (best_total) best_total[e] = P > 0 ? totals[b] : 0.f;
    }
  }
  if (total)
    for (int k = wave * NTL + lane; k < K; k += WAVES * NTL) total[(size_t)e * K + k] = P > 0 ? totals[k / leaves] : 0.f;
  for (int ft = wave; ft < F * H; ft += WAVES) {   // rows t >= steps: zeros
    const int t = ft % H;
    const size_t row = (size_t)e * F * H + ft;
    if (level_plans) level_plans[row * NTL + lane] = t < steps ? sh.plans[ft * NTL + lane] : 0;
    if (level_bytes && lane == 0) level_bytes[row] = t < steps ? sh.chunk_size[ft] : 0;
  }
}

// Model::client == false is mansy_sim_drive: the look-ahead on the trace and the ground truth, the last sample as the estimate; the
// arguments from `network` on are not read.  true: the look-ahead scores on vmap with the network model `network`, and the estimate
// comes from the window of samples (history f64 [n,8], count i32 [n], in and out).
// Model::schedules (mansy_sim_drive_schedules): the client's loop with fractions = the K budget levels, one of which every step of a
// candidate takes: sched_search stands in for the allocations and the walks, wave 0 scans the totals of the prefixes and commits the
// first step of the winner's first level.  The dynamic LDS is then K^H totals alone; the K x H plans live in the static part.
template <int WAVES, typename Model>
__global__ __launch_bounds__(WAVES * 64) void sim_drive_kernel(mansy_env_tables T, EnvState* st, const double* __restrict__ fractions, int K, int H, int D,
                                                               double* throughput, int* best, float* best_total, int* versions, float* qoe_parts,
                                                               double* scalars, unsigned char* over_out, int auto_reset, int network,
                                                               const unsigned char* __restrict__ vmap, int window, double* history, int* count) {
  extern __shared__ __align__(16) unsigned char drive_lds[];
  __shared__ typename Model::Shared sh;
  float* totals = (float*)drive_lds;
  unsigned char* plans;
  if constexpr (Model::schedules) plans = sh.plans; else plans = drive_lds + sizeof(float) * K;
  const int e = blockIdx.x, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  bool moved = false, sampled = false;        // wave 0's alone
  int schedules = 1;                          // Model::schedules: K^H, the schedules of K levels
  if constexpr (Model::schedules) for (int h = 0; h < H; ++h) schedules *= K;
  if (wave == 0) {
    EnvRegs s;
    load_state(s, st[e], lane);
    store_state(sh.rec, s, lane);
    if (lane == 0) sh.throughput = throughput[e];
    if constexpr (Model::client) {
      if (lane < MANSY_SIM_EST_MAX_WINDOW) sh.history[lane] = history[(size_t)e * MANSY_SIM_EST_MAX_WINDOW + lane];
      if (lane == 0) { const int c = count[e]; sh.count = c < 0 ? 0 : c > MANSY_SIM_EST_MAX_WINDOW ? MANSY_SIM_EST_MAX_WINDOW : c; }
    }
  }
  __syncthreads();
  for (int d = 0; d < D; ++d) {
    SessionView v = view_of(sh.rec);          // the same values in every lane of the workgroup; the integers into scalar registers
    v.video = __builtin_amdgcn_readfirstlane(v.video); v.vp = __builtin_amdgcn_readfirstlane(v.vp);
    v.trace = __builtin_amdgcn_readfirstlane(v.trace); v.qoe = __builtin_amdgcn_readfirstlane(v.qoe);
    v.next_chunk = __builtin_amdgcn_readfirstlane(v.next_chunk); v.end_chunk = __builtin_amdgcn_readfirstlane(v.end_chunk);
    v.cur_idx = __builtin_amdgcn_readfirstlane(v.cur_idx); v.has_prev = __builtin_amdgcn_readfirstlane(v.has_prev);
    const int steps = steps_ahead(T, v.next_chunk, v.end_chunk, H);          // 0: a closed record, nothing to plan
    const double thr = sh.throughput;
    int P = K;                                // the totals wave 0 scans: one per candidate, or one per schedule prefix
    if constexpr (Model::schedules) {
      P = sched_search<WAVES>(T, v, steps, thr, fractions, K, H, network, vmap, sh, totals, wave, lane);
    } else {
      drive_allocate<WAVES>(T, v, steps, thr * (double)T.chunk_length, fractions, K, H, plans, sh, wave, lane);
      if (steps > 0) {
        for (int k = wave; k < K; k += WAVES) {
          const PlanBytes plan = {plans + k * H * NTL + lane};
          float sum;
          if constexpr (Model::client) {       // (network is a kernel argument: the whole workgroup takes the same side)
            sum = network == NET_ESTIMATE ? look_walk<NET_ESTIMATE>(T, v, steps, plan, lane, thr, vmap, nullptr, nullptr)
                                          : look_walk<NET_TRACE>(T, v, steps, plan, lane, 0.0, vmap, nullptr, nullptr);
          } else {
            sum = look_walk<NET_TRACE>(T, v, steps, plan, lane, 0.0, T.vp_gt, nullptr, nullptr);
          }
          if (lane == 0) totals[k] = sum;
        }
      }
      __syncthreads();
    }
    if (wave == 0) {
      const size_t row = (size_t)e * D + d;
      int b = 0, ver = 0;
      float bt = 0.f;                         // a closed record: plans and totals are zeros, candidate 0
      if (steps > 0) {
        b = best_of(totals, P, lane); bt = totals[b];
        if constexpr (Model::schedules) {      // K levels: prefix b begins with level b / K^(steps-1) and is schedule b x K^(H-steps)
          ver = plans[b / (P / K) * H * NTL + lane];
          b *= schedules / P;
        } else {
          ver = plans[b * H * NTL + lane];
        }
      }
      if (lane == 0) {
        if (best) best[row] = b;
        if (best_total) best_total[row] = bt;
      }
      if (versions) versions[row * NTL + lane] = ver;
      if (steps == 0 && !auto_reset) {        // sim_download_kernel's closed path: zeros, and the record stays as it is
        if (lane < 4) {
          if (scalars) scalars[4 * row + lane] = 0.0;
          if (qoe_parts) qoe_parts[4 * row + lane] = 0.f;
        }
        if (lane == 0) over_out[row] = 1;
      } else {
        EnvRegs s;
        load_state(s, sh.rec, lane);
        if (steps == 0) do_reset(T, s);
        const Committed c = sim_commit(T, s, ver, lane, nullptr, nullptr, nullptr, scalars ? scalars + 4 * row : nullptr,
                                       qoe_parts ? qoe_parts + 4 * row : nullptr, over_out + row, auto_reset);
        store_state(sh.rec, s, lane);
        if constexpr (Model::client) {
          if (c.download_time > 0) {           // (wave-uniform)
            if (lane == 0) {
              int cnt = sh.count;
              sh.throughput = estimate_push(sh.history, cnt, (double)c.chunk_size / c.download_time, window);
              sh.count = cnt;
            }
            sampled = true;
          }
        } else {
          if (lane == 0) sh.throughput = c.download_time > 0 ? (double)c.chunk_size / c.download_time : thr;
        }
        moved = true;
      }
    }
    __syncthreads();
  }
  if (wave == 0) {
    if (moved) {
      EnvRegs s;
      load_state(s, sh.rec, lane);
      store_state(st[e], s, lane);
    }
    if (lane == 0) throughput[e] = sh.throughput;
    if constexpr (Model::client) {
      if (sampled) {                          // the slots and the count go back once, if a step gave a sample
        if (lane < MANSY_SIM_EST_MAX_WINDOW) history[(size_t)e * MANSY_SIM_EST_MAX_WINDOW + lane] = sh.history[lane];
        if (lane == 0) count[e] = sh.count;
      }
    }
  }
}

int check_sim_tables(const mansy_env_tables* T, const char* who) {   // the conditions env.hip's check_tables makes
  MANSY_REQUIRE(T, "%s: null tables", who);
  MANSY_REQUIRE(T->size && T->quality && T->video_len && T->vp_gt && T->vp_pred && T->vp_acc && T->vp_start && T->vp_end && T->trace_bw &&
                    T->trace_len && T->samples && T->qoe_w, "%s: null table pointer", who);
  MANSY_REQUIRE(T->n_sample >= 1 && T->n_chunk_max >= 1 && T->n_vpchunk_max >= 1 && T->trace_len_max >= 1, "%s: empty tables", who);
  return MANSY_OK;
}

}  // namespace

extern "C" {

int mansy_sim_download(const mansy_env_tables* T, void* state, int n, const int* tile_rates, float* tile_size, float* tile_quality,
                       unsigned char* actual_viewport, double* scalars, float* qoe_parts, unsigned char* over, int auto_reset, void* stream) {
  int rc = check_sim_tables(T, "sim_download"); if (rc) return rc;
  MANSY_REQUIRE(state, "sim_download: null state");
  MANSY_REQUIRE(tile_rates, "sim_download: null tile_rates");
  MANSY_REQUIRE(over, "sim_download: null over");
  MANSY_REQUIRE(n >= 1, "sim_download: n must be >= 1");
  MANSY_LAUNCH(sim_download_kernel, dim3(mansy_ceil_div((long long)n * 64, 256)), dim3(256), 0, (hipStream_t)stream, *T, (EnvState*)state, n,
               tile_rates, tile_size, tile_quality, actual_viewport, scalars, qoe_parts, over, auto_reset);
  MANSY_LAUNCH_CHECK();
  return MANSY_OK;
}

int mansy_sim_peek(const mansy_env_tables* T, const void* state, int n, int* next_chunk, double* buffer, float* size, float* quality,
                   unsigned char* gt, unsigned char* pred, double* acc, void* stream) {
  int rc = check_sim_tables(T, "sim_peek"); if (rc) return rc;
  MANSY_REQUIRE(state, "sim_peek: null state");
  MANSY_REQUIRE(n >= 1, "sim_peek: n must be >= 1");
  MANSY_LAUNCH(sim_peek_kernel, dim3(mansy_ceil_div((long long)n * 64, 256)), dim3(256), 0, (hipStream_t)stream, *T, (const EnvState*)state, n,
               next_chunk, buffer, size, quality, gt, pred, acc);
  MANSY_LAUNCH_CHECK();
  return MANSY_OK;
}

int mansy_sim_lookahead(const mansy_env_tables* T, const void* state, int n, const int* plans, int K, int H, float* qoe_parts,
                        double* scalars, float* total, int* steps, int* best, float* best_total, void* stream) {
  int rc = check_sim_tables(T, "sim_lookahead"); if (rc) return rc;
  MANSY_REQUIRE(state, "sim_lookahead: null state");
  MANSY_REQUIRE(plans, "sim_lookahead: null plans");
  MANSY_REQUIRE(total, "sim_lookahead: null total");
  MANSY_REQUIRE(steps, "sim_lookahead: null steps");
  MANSY_REQUIRE(n >= 1, "sim_lookahead: n must be >= 1");
  MANSY_REQUIRE(K >= 1 && K <= MANSY_SIM_MAX_CANDIDATES, "sim_lookahead: K must be in [1, %d]", MANSY_SIM_MAX_CANDIDATES);
  MANSY_REQUIRE(H >= 1 && H <= MANSY_SIM_MAX_HORIZON, "sim_lookahead: H must be in [1, %d]", MANSY_SIM_MAX_HORIZON);
  MANSY_REQUIRE((long long)n * K < (1ll << 31), "sim_lookahead: n * K must be below 2^31");
  MANSY_LAUNCH(sim_lookahead_kernel<NET_TRACE>, dim3((unsigned)mansy_ceil_div((long long)n * K * 64, 256)), dim3(256), 0, (hipStream_t)stream, *T,
               (const EnvState*)state, n, plans, K, H, (const double*)nullptr, T->vp_gt, qoe_parts, scalars, total, steps);
  if (best || best_total)
    MANSY_LAUNCH(sim_best_kernel, dim3(mansy_ceil_div((long long)n * 64, 256)), dim3(256), 0, (hipStream_t)stream, total, n, K, best, best_total);
  MANSY_LAUNCH_CHECK();
  return MANSY_OK;
}

int mansy_sim_lookahead_client(const mansy_env_tables* T, const void* state, int n, const int* plans, int K, int H, const double* throughput,
                               int viewport, float* qoe_parts, double* scalars, float* total, int* steps, int* best, float* best_total,
                               void* stream) {
  int rc = check_sim_tables(T, "sim_lookahead_client"); if (rc) return rc;
  MANSY_REQUIRE(state, "sim_lookahead_client: null state");
  MANSY_REQUIRE(plans, "sim_lookahead_client: null plans");
  MANSY_REQUIRE(total, "sim_lookahead_client: null total");
  MANSY_REQUIRE(steps, "sim_lookahead_client: null steps");
  MANSY_REQUIRE(n >= 1, "sim_lookahead_client: n must be >= 1");
  MANSY_REQUIRE(K >= 1 && K <= MANSY_SIM_MAX_CANDIDATES, "sim_lookahead_client: K must be in [1, %d]", MANSY_SIM_MAX_CANDIDATES);
  MANSY_REQUIRE(H >= 1 && H <= MANSY_SIM_MAX_HORIZON, "sim_lookahead_client: H must be in [1, %d]", MANSY_SIM_MAX_HORIZON);
  MANSY_REQUIRE((long long)n * K < (1ll << 31), "sim_lookahead_client: n * K must be below 2^31");
  MANSY_REQUIRE(viewport == MANSY_SIM_VIEW_GT || viewport == MANSY_SIM_VIEW_PRED, "sim_lookahead_client: viewport must be MANSY_SIM_VIEW_GT (0) or MANSY_SIM_VIEW_PRED (1)");
  const unsigned char* vmap = viewport == MANSY_SIM_VIEW_PRED ? T->vp_pred : T->vp_gt;
  const dim3 grid((unsigned)mansy_ceil_div((long long)n * K * 64, 256));
  if (throughput)
    MANSY_LAUNCH(sim_lookahead_kernel<NET_ESTIMATE>, grid, dim3(256), 0, (hipStream_t)stream, *T, (const EnvState*)state, n, plans, K, H, throughput, vmap,
                 qoe_parts, scalars, total, steps);
  else
    MANSY_LAUNCH(sim_lookahead_kernel<NET_TRACE>, grid, dim3(256), 0, (hipStream_t)stream, *T, (const EnvState*)state, n, plans, K, H, throughput, vmap,
                 qoe_parts, scalars, total, steps);
  if (best || best_total)
    MANSY_LAUNCH(sim_best_kernel, dim3(mansy_ceil_div((long long)n * 64, 256)), dim3(256), 0, (hipStream_t)stream, total, n, K, best, best_total);
  MANSY_LAUNCH_CHECK();
  return MANSY_OK;
}

int mansy_sim_allocate(const mansy_env_tables* T, const void* state, int n, const double* budgets, const float* weights, int K, int H,
                       int* plans, int* plan_bytes, int* steps, void* stream) {
  int rc = check_sim_tables(T, "sim_allocate"); if (rc) return rc;
  MANSY_REQUIRE(state, "sim_allocate: null state");
  MANSY_REQUIRE(budgets, "sim_allocate: null budgets");
  MANSY_REQUIRE(plans, "sim_allocate: null plans");
  MANSY_REQUIRE(steps, "sim_allocate: null steps");
  MANSY_REQUIRE(n >= 1, "sim_allocate: n must be >= 1");
  MANSY_REQUIRE(K >= 1 && K <= MANSY_SIM_MAX_CANDIDATES, "sim_allocate: K must be in [1, %d]", MANSY_SIM_MAX_CANDIDATES);
  MANSY_REQUIRE(H >= 1 && H <= MANSY_SIM_MAX_HORIZON, "sim_allocate: H must be in [1, %d]", MANSY_SIM_MAX_HORIZON);
  MANSY_REQUIRE((long long)n * K * H < (1ll << 31), "sim_allocate: n * K * H must be below 2^31");
  MANSY_LAUNCH(sim_allocate_kernel, dim3((unsigned)mansy_ceil_div((long long)n * K * H * 64, 256)), dim3(256), 0, (hipStream_t)stream, *T,
               (const EnvState*)state, n, budgets, weights, K, H, plans, plan_bytes, steps);
  MANSY_LAUNCH_CHECK();
  return MANSY_OK;
}

int mansy_sim_drive(const mansy_env_tables* T, void* state, int n, const double* fractions, int K, int H, int D, double* throughput, int* best,
                    float* best_total, int* versions, float* qoe_parts, double* scalars, unsigned char* over, int auto_reset, void* stream) {
  int rc = check_sim_tables(T, "sim_drive"); if (rc) return rc;
  MANSY_REQUIRE(state, "sim_drive: null state");
  MANSY_REQUIRE(fractions, "sim_drive: null fractions");
  MANSY_REQUIRE(throughput, "sim_drive: null throughput");
  MANSY_REQUIRE(over, "sim_drive: null over");
  MANSY_REQUIRE(n >= 1, "sim_drive: n must be >= 1");
  MANSY_REQUIRE(K >= 1 && K <= MANSY_SIM_DRIVE_MAX_CANDIDATES, "sim_drive: K must be in [1, %d]", MANSY_SIM_DRIVE_MAX_CANDIDATES);
  MANSY_REQUIRE(H >= 1 && H <= MANSY_SIM_MAX_HORIZON, "sim_drive: H must be in [1, %d]", MANSY_SIM_MAX_HORIZON);
  MANSY_REQUIRE(D >= 1 && D <= MANSY_SIM_DRIVE_MAX_DECISIONS, "sim_drive: D must be in [1, %d]", MANSY_SIM_DRIVE_MAX_DECISIONS);
  const size_t lds = sizeof(float) * K + (size_t)K * H * NTL;      // the totals, then the plans as bytes
  // few sessions: sixteen waves each, so that every CU works on the one session it holds; many: four, so that a CU holds several
  // sessions whose serial parts (the leading allocations, the commit) overlap (DESIGN.md section 1 has the measurement)
  if (n <= DRIVE_WIDE_SESSIONS)
    MANSY_LAUNCH((sim_drive_kernel<16, DriveOracle>), dim3((unsigned)n), dim3(16 * 64), lds, (hipStream_t)stream, *T, (EnvState*)state, fractions, K, H, D,
                 throughput, best, best_total, versions, qoe_parts, scalars, over, auto_reset, NET_TRACE, T->vp_gt, 1, (double*)nullptr, (int*)nullptr);
  else
    MANSY_LAUNCH((sim_drive_kernel<4, DriveOracle>), dim3((unsigned)n), dim3(4 * 64), lds, (hipStream_t)stream, *T, (EnvState*)state, fractions, K, H, D,
                 throughput, best, best_total, versions, qoe_parts, scalars, over, auto_reset, NET_TRACE, T->vp_gt, 1, (double*)nullptr, (int*)nullptr);
  MANSY_LAUNCH_CHECK();
  return MANSY_OK;
}

int mansy_sim_drive_client(const mansy_env_tables* T, void* state, int n, const double* fractions, int K, int H, int D, double* throughput,
                           int network, int viewport, int window, double* history, int* count, int* best, float* best_total, int* versions,
                           float* qoe_parts, double* scalars, unsigned char* over, int auto_reset, void* stream) {
  int rc = check_sim_tables(T, "sim_drive_client"); if (rc) return rc;
  MANSY_REQUIRE(state, "sim_drive_client: null state");
  MANSY_REQUIRE(fractions, "sim_drive_client: null fractions");
  MANSY_REQUIRE(throughput, "sim_drive_client: null throughput");
  MANSY_REQUIRE(history, "sim_drive_client: null history");
  MANSY_REQUIRE(count, "sim_drive_client: null count");
  MANSY_REQUIRE(over, "sim_drive_client: null over");
  MANSY_REQUIRE(n >= 1, "sim_drive_client: n must be >= 1");
  MANSY_REQUIRE(K >= 1 && K <= MANSY_SIM_DRIVE_MAX_CANDIDATES, "sim_drive_client: K must be in [1, %d]", MANSY_SIM_DRIVE_MAX_CANDIDATES);
  MANSY_REQUIRE(H >= 1 && H <= MANSY_SIM_MAX_HORIZON, "sim_drive_client: H must be in [1, %d]", MANSY_SIM_MAX_HORIZON);
  MANSY_REQUIRE(D >= 1 && D <= MANSY_SIM_DRIVE_MAX_DECISIONS, "sim_drive_client: D must be in [1, %d]", MANSY_SIM_DRIVE_MAX_DECISIONS);
  MANSY_REQUIRE(network == MANSY_SIM_NET_TRACE || network == MANSY_SIM_NET_ESTIMATE, "sim_drive_client: network must be MANSY_SIM_NET_TRACE (0) or MANSY_SIM_NET_ESTIMATE (1)");
  MANSY_REQUIRE(viewport == MANSY_SIM_VIEW_GT || viewport == MANSY_SIM_VIEW_PRED, "sim_drive_client: viewport must be MANSY_SIM_VIEW_GT (0) or MANSY_SIM_VIEW_PRED (1)");
  MANSY_REQUIRE(window >= 1 && window <= MANSY_SIM_EST_MAX_WINDOW, "sim_drive_client: window must be in [1, %d]", MANSY_SIM_EST_MAX_WINDOW);
  const unsigned char* vmap = viewport == MANSY_SIM_VIEW_PRED ? T->vp_pred : T->vp_gt;
  const size_t lds = sizeof(float) * K + (size_t)K * H * NTL;      // as mansy_sim_drive's, and the same two workgroup widths
  if (n <= DRIVE_WIDE_SESSIONS)
    MANSY_LAUNCH((sim_drive_kernel<16, DriveClient>), dim3((unsigned)n), dim3(16 * 64), lds, (hipStream_t)stream, *T, (EnvState*)state, fractions, K, H, D,
                 throughput, best, best_total, versions, qoe_parts, scalars, over, auto_reset, network, vmap, window, history, count);
  else
    MANSY_LAUNCH((sim_drive_kernel<4, DriveClient>), dim3((unsigned)n), dim3(4 * 64), lds, (hipStream_t)stream, *T, (EnvState*)state, fractions, K, H, D,
                 throughput, best, best_total, versions, qoe_parts, scalars, over, auto_reset, network, vmap, window, history, count);
  MANSY_LAUNCH_CHECK();
  return MANSY_OK;
}

// F^H where it is at most MANSY_SIM_MAX_CANDIDATES, 0 otherwise (F and H within their own limits).
static int schedule_count(int F, int H) {
  long long K = 1;
  for (int h = 0; h < H; ++h) { K *= F; if (K > MANSY_SIM_MAX_CANDIDATES) return 0; }
  return (int)K;
}

int mansy_sim_lookahead_schedules(const mansy_env_tables* T, const void* state, int n, const double* levels, int F, int H,
                                  const double* throughput, int network, int viewport, int* level_plans, int* level_bytes, float* total,
                                  int* steps, int* best, float* best_total, void* stream) {
  int rc = check_sim_tables(T, "sim_lookahead_schedules"); if (rc) return rc;
  MANSY_REQUIRE(state, "sim_lookahead_schedules: null state");
  MANSY_REQUIRE(levels, "sim_lookahead_schedules: null levels");
  MANSY_REQUIRE(throughput, "sim_lookahead_schedules: null throughput");
  MANSY_REQUIRE(steps, "sim_lookahead_schedules: null steps");
  MANSY_REQUIRE(n >= 1, "sim_lookahead_schedules: n must be >= 1");
  MANSY_REQUIRE(F >= 1 && F <= MANSY_SIM_SCHED_MAX_LEVELS, "sim_lookahead_schedules: F must be in [1, %d]", MANSY_SIM_SCHED_MAX_LEVELS);
  MANSY_REQUIRE(H >= 1 && H <= MANSY_SIM_MAX_HORIZON, "sim_lookahead_schedules: H must be in [1, %d]", MANSY_SIM_MAX_HORIZON);
  const int K = schedule_count(F, H);
  MANSY_REQUIRE(K >= 1, "sim_lookahead_schedules: F^H must be at most %d", MANSY_SIM_MAX_CANDIDATES);
  MANSY_REQUIRE((long long)n * K < (1ll << 31), "sim_lookahead_schedules: n * F^H must be below 2^31");
  MANSY_REQUIRE(network == MANSY_SIM_NET_TRACE || network == MANSY_SIM_NET_ESTIMATE, "sim_lookahead_schedules: network must be MANSY_SIM_NET_TRACE (0) or MANSY_SIM_NET_ESTIMATE (1)");
  MANSY_REQUIRE(viewport == MANSY_SIM_VIEW_GT || viewport == MANSY_SIM_VIEW_PRED, "sim_lookahead_schedules: viewport must be MANSY_SIM_VIEW_GT (0) or MANSY_SIM_VIEW_PRED (1)");
  const unsigned char* vmap = viewport == MANSY_SIM_VIEW_PRED ? T->vp_pred : T->vp_gt;
  const size_t lds = sizeof(float) * K;                            // the totals; mansy_sim_drive's two workgroup widths
  if (n <= DRIVE_WIDE_SESSIONS)
    MANSY_LAUNCH(sim_lookahead_schedules_kernel<16>, dim3((unsigned)n), dim3(16 * 64), lds, (hipStream_t)stream, *T, (const EnvState*)state, levels, F, H, K,
                 throughput, network, vmap, level_plans, level_bytes, total, steps, best, best_total);
  else
    MANSY_LAUNCH(sim_lookahead_schedules_kernel<4>, dim3((unsigned)n), dim3(4 * 64), lds, (hipStream_t)stream, *T, (const EnvState*)state, levels, F, H, K,
                 throughput, network, vmap, level_plans, level_bytes, total, steps, best, best_total);
  MANSY_LAUNCH_CHECK();
  return MANSY_OK;
}

int mansy_sim_drive_schedules(const mansy_env_tables* T, void* state, int n, const double* levels, int F, int H, int D, double* throughput,
                              int network, int viewport, int window, double* history, int* count, int* best, float* best_total,
                              int* versions, float* qoe_parts, double* scalars, unsigned char* over, int auto_reset, void* stream) {
  int rc = check_sim_tables(T, "sim_drive_schedules"); if (rc) return rc;
  MANSY_REQUIRE(state, "sim_drive_schedules: null state");
  MANSY_REQUIRE(levels, "sim_drive_schedules: null levels");
  MANSY_REQUIRE(throughput, "sim_drive_schedules: null throughput");
  MANSY_REQUIRE(history, "sim_drive_schedules: null history");
  MANSY_REQUIRE(count, "sim_drive_schedules: null count");
  MANSY_REQUIRE(over, "sim_drive_schedules: null over");
  MANSY_REQUIRE(n >= 1, "sim_drive_schedules: n must be >= 1");
  MANSY_REQUIRE(F >= 1 && F <= MANSY_SIM_SCHED_MAX_LEVELS, "sim_drive_schedules: F must be in [1, %d]", MANSY_SIM_SCHED_MAX_LEVELS);
  MANSY_REQUIRE(H >= 1 && H <= MANSY_SIM_MAX_HORIZON, "sim_drive_schedules: H must be in [1, %d]", MANSY_SIM_MAX_HORIZON);
  const int K = schedule_count(F, H);
  MANSY_REQUIRE(K >= 1, "sim_drive_schedules: F^H must be at most %d", MANSY_SIM_MAX_CANDIDATES);
  MANSY_REQUIRE((long long)n * K < (1ll << 31), "sim_drive_schedules: n * F^H must be below 2^31");
  MANSY_REQUIRE(D >= 1 && D <= MANSY_SIM_DRIVE_MAX_DECISIONS, "sim_drive_schedules: D must be in [1, %d]", MANSY_SIM_DRIVE_MAX_DECISIONS);
  MANSY_REQUIRE(network == MANSY_SIM_NET_TRACE || network == MANSY_SIM_NET_ESTIMATE, "sim_drive_schedules: network must be MANSY_SIM_NET_TRACE (0) or MANSY_SIM_NET_ESTIMATE (1)");
  MANSY_REQUIRE(viewport == MANSY_SIM_VIEW_GT || viewport == MANSY_SIM_VIEW_PRED, "sim_drive_schedules: viewport must be MANSY_SIM_VIEW_GT (0) or MANSY_SIM_VIEW_PRED (1)");
  MANSY_REQUIRE(window >= 1 && window <= MANSY_SIM_EST_MAX_WINDOW, "sim_drive_schedules: window must be in [1, %d]", MANSY_SIM_EST_MAX_WINDOW);
  const unsigned char* vmap = viewport == MANSY_SIM_VIEW_PRED ? T->vp_pred : T->vp_gt;
  const size_t lds = sizeof(float) * K;                            // the totals of the schedules; the kernel's K is the number of levels
  if (n <= DRIVE_WIDE_SESSIONS)
    MANSY_LAUNCH((sim_drive_kernel<16, DriveSchedules>), dim3((unsigned)n), dim3(16 * 64), lds, (hipStream_t)stream, *T, (EnvState*)state, levels, F, H, D,
                 throughput, best, best_total, versions, qoe_parts, scalars, over, auto_reset, network, vmap, window, history, count);
  else
    MANSY_LAUNCH((sim_drive_kernel<4, DriveSchedules>), dim3((unsigned)n), dim3(4 * 64), lds, (hipStream_t)stream, *T, (EnvState*)state, levels, F, H, D,
                 throughput, best, best_total, versions, qoe_parts, scalars, over, auto_reset, network, vmap, window, history, count);
  MANSY_LAUNCH_CHECK();
  return MANSY_OK;
}

int mansy_sim_peek_ahead(const mansy_env_tables* T, const void* state, int n, int ahead, float* size, float* quality, unsigned char* gt,
                         unsigned char* pred, double* acc, unsigned char* valid, void* stream) {
  int rc = check_sim_tables(T, "sim_peek_ahead"); if (rc) return rc;
  MANSY_REQUIRE(state, "sim_peek_ahead: null state");
  MANSY_REQUIRE(valid, "sim_peek_ahead: null valid");
  MANSY_REQUIRE(n >= 1, "sim_peek_ahead: n must be >= 1");
  MANSY_REQUIRE(ahead >= 0 && ahead < MANSY_SIM_MAX_HORIZON, "sim_peek_ahead: ahead must be in [0, %d)", MANSY_SIM_MAX_HORIZON);
  MANSY_LAUNCH(sim_peek_ahead_kernel, dim3(mansy_ceil_div((long long)n * 64, 256)), dim3(256), 0, (hipStream_t)stream, *T, (const EnvState*)state, n,
               ahead, size, quality, gt, pred, acc, valid);
  MANSY_LAUNCH_CHECK();
  return MANSY_OK;
}

}  // extern "C"
