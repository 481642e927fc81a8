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
#include "mansy_kernels.h"
#include "../../include/mansy_hip.h"

#pragma clang fp contract(off)

namespace {

#include "env_device.h"

// A record no session is open in: past its last chunk, or never reset since mansy_env_init (next_chunk == 0 there).
__device__ __forceinline__ bool session_closed(const mansy_env_tables& T, int next_chunk, int end_chunk) {
  return next_chunk > end_chunk || next_chunk <= T.startup_download;
}

__device__ __forceinline__ double seq_dsum64(float x) {      // ((..(0 + x0) + x1) ..) + x63 in float64, tile order (Python sum of a list)
  double s = 0.0;
#pragma unroll
  for (int t = 0; t < NTL; ++t) s = s + (double)__builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), t));
  return s;
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
  const int chunk = s.next_chunk;
  // ---- loads that depend on the state alone
  int ver = tile_rates[row];
  ver = ver < 0 ? 0 : ver > NR - 1 ? NR - 1 : ver;
  const size_t mrow = ((size_t)s.video * T.n_chunk_max + chunk) * NR * NTL;
  int size_r[NR]; float qual_r[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) { size_r[r] = T.size[mrow + r * NTL + lane]; qual_r[r] = T.quality[mrow + r * NTL + lane]; }
  const size_t vrow = ((size_t)s.vp * T.n_vpchunk_max + (chunk - T.vp_start[s.vp])) * NTL;
  const unsigned char gt = T.vp_gt[vrow + lane];
  const float gv = (float)gt;
  const float* w = T.qoe_w + 3 * s.qoe;
  const float w0 = w[0], w1 = w[1], w2 = w[2];
  const double* bw = T.trace_bw + (size_t)s.trace * T.trace_len_max;
  const int tlen = T.trace_len[s.trace];
  double bwc = bw[s.cur_idx];
  const bool over_pre = chunk + 1 > s.end_chunk;
  const double acc_next = over_pre ? 0.0 : T.vp_acc[(size_t)s.vp * T.n_vpchunk_max + (chunk + 1 - T.vp_start[s.vp])];
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
  if (tile_size) tile_size[row] = (float)my_size;
  if (tile_quality) tile_quality[row] = tq;
  if (actual_viewport) actual_viewport[row] = gt;
  if (scalars) {                             // (a launch-uniform branch: the 64-term double chain is skipped when nobody asks)
    const double chunk_quality = seq_dsum64(tq);
    if (lane == 0) {
      scalars[4 * e + 0] = (double)chunk_size; scalars[4 * e + 1] = chunk_quality; scalars[4 * e + 2] = download_time; scalars[4 * e + 3] = rebuf;
    }
  }
  if (lane == 0) {
    if (qoe_parts) { qoe_parts[4 * e + 0] = qoe; qoe_parts[4 * e + 1] = qoe1; qoe_parts[4 * e + 2] = (float)rebuf; qoe_parts[4 * e + 3] = qoe3; }
    over_out[e] = over ? 1 : 0;
  }
  if (over && auto_reset) do_reset(T, s);    // the session opens its next catalogue entry, as the vector environment does
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
  const size_t mrow = ((size_t)video * T.n_chunk_max + chunk) * NR * NTL;
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    if (size) size[((size_t)e * NR + r) * NTL + lane] = (float)T.size[mrow + r * NTL + lane];
    if (quality) quality[((size_t)e * NR + r) * NTL + lane] = T.quality[mrow + r * NTL + lane];
  }
  const size_t vrow = ((size_t)vp * T.n_vpchunk_max + (chunk - T.vp_start[vp])) * NTL;
  if (gt) gt[row] = T.vp_gt[vrow + lane];
  if (pred) pred[row] = T.vp_pred[vrow + lane];
}

int check_sim_tables(const mansy_env_tables* T, const char* who) {     // the conditions env.hip's check_tables makes
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

}  // extern "C"
