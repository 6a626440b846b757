// Per-env episodes inside the rollout kernel (include/mds.h mds_rollout_episodes; the rule: mds_episode.hpp).
//
// k_rollout_episodes is k_rollout_step -- n_steps control steps per launch with the state in registers, a replayed action table, an
// observation log ring -- composed from the same per-drone pieces (load_state, aviary_step_any, pack_obs, write_obs_rows,
// store_state), plus, after every step: the drone's cause bits and reward term, their OR / sum over the drones of the env, the env's
// reward and flags into their log rings, the env's counters, and for a done env every drone back to its row of the reset image.
//
// Thread mapping.  The flat mapping of the other kernels (drone i = block * 256 + thread) lets an env straddle waves and workgroups
// whenever D does not divide 64.  Here a workgroup owns episode_envs_per_block(D) whole envs: drone i = block * (envs * D) + thread,
// the tail lanes idle.  The env's OR and sum go through LDS: every lane publishes its two values, one workgroup barrier, every lane
// reads the D values of its env (so each lane knows `done` without a second barrier; the buffers alternate by step parity, which is
// what lets one barrier per step suffice: a wave can be at most one barrier ahead of another).
// write_obs_rows needs a wave's rows to be one contiguous span starting at i - lane (they are: 64 consecutive threads, consecutive
// drones), bounded by its `n` argument (the block's end), and, for the 40-byte fp16 rows, an even first drone in every wave: the
// envs per block are chosen so that envs * D is even.
#include "mds_episode.hpp"

namespace mds {

// envs a workgroup owns: as many as fit, one fewer where that makes the block's drone count even (D <= kBlock / 2)
__host__ __device__ __forceinline__ int episode_envs_per_block(int D) {
  int e = kBlock / D;
  if (e > 1 && ((e * D) & 1)) --e;
  return e;
}

// per-env counters: the running episode's length and return, and of the completed episodes their number, summed returns, summed lengths
template <typename T> struct EpisodeCounters {
  int* length;
  T* ret;
  int* count;
  T* sum_return;
  int* sum_length;
};

// target planes [3][ld] in the local frame: the caller's world-frame target less the origin, or (target_world NULL) the reset position
template <typename T, typename S>
__global__ void k_episode_targets(const int n, const size_t ld, const double* __restrict__ target_world, const T* __restrict__ origin,
                                  const S* __restrict__ image, T* __restrict__ target) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  for (int k = 0; k < 3; ++k)
    target[k * ld + i] = target_world ? (T)(target_world[3 * (size_t)i + k] - (double)origin[k * ld + i]) : (T)image[sidx(k, i, ld)];
}

template <typename T, typename S, bool RK4, bool DRAG>
__global__ __launch_bounds__(kBlock) void k_rollout_episodes(const Consts<T> c, const EpisodeRule<T> rule, const int n, const size_t ld, const int D,
                                                             const int envs_per_block, S* __restrict__ state, const S* __restrict__ image,
                                                             const T* __restrict__ origin, const T* __restrict__ target, T* __restrict__ last_rpm,
                                                             const S* __restrict__ actions, int a0, const int n_sets, S* __restrict__ obs_log,
                                                             T* __restrict__ reward_log, int* __restrict__ flags_log, int s0, const int n_slots,
                                                             const int n_steps, S* __restrict__ obs_now, const EpisodeCounters<T> cnt) {
  __shared__ __align__(16) unsigned char lds[kBlock * kObsDim * sizeof(S)];
  __shared__ int red_cause[2][kBlock];
  __shared__ T red_term[2][kBlock];
  const int tid = (int)threadIdx.x;
  const int per_block = envs_per_block * D;
  const int first = (int)blockIdx.x * per_block;
  const int i = first + tid;
  const int block_end = min(first + per_block, n);          // n = E * D: whole envs
  const bool valid = tid < per_block && i < n;
  const int le = tid / D, d = tid - le * D;                 // env within the block, drone within the env
  const int E = n / D, e = (int)blockIdx.x * envs_per_block + le;
  State<T> s;
  Resid<T> r;
  resid_zero(r);
  V3<T> org = {T(0), T(0), T(0)}, home = org, tgt = org;
  T prev[4] = {T(0), T(0), T(0), T(0)}, clipped[4] = {T(0), T(0), T(0), T(0)};
  int length = 0, count = 0, sum_length = 0;
  T ret = T(0), sum_return = T(0);
  if (valid) {
    load_state<S, T>(state, ld, i, s);
    org = load_origin(origin, ld, i);
    home = {(T)image[sidx(0, i, ld)], (T)image[sidx(1, i, ld)], (T)image[sidx(2, i, ld)]};
    tgt = load_origin(target, ld, i);       // (held across the loop: reloading both per step frees no register and measured no faster)
    if (DRAG)
      for (int k = 0; k < 4; ++k) prev[k] = last_rpm[k * ld + i];
    length = cnt.length[e]; ret = cnt.ret[e];
    count = cnt.count[e]; sum_return = cnt.sum_return[e]; sum_length = cnt.sum_length[e];
  }
  for (int k = 0; k < n_steps; ++k) {
    T o[kObsDim];
    int cause = 0;
    T term = T(0);
    if (valid) {
      T act[4];
      load4<S, T>(actions + ((size_t)a0 * n + i) * 4, act);
      aviary_step_any<T, RK4, DRAG, false>(c, s, r, act, prev, clipped);
      if (obs_log != nullptr) pack_obs(s, org, clipped, o);
      cause = episode_causes(rule, s, s.p.z + org.z, home);
      term = episode_reward_term(rule, s.p, tgt);
    }
    // the logged row is the transition's result: before any reset
    if (obs_log != nullptr) write_obs_rows<S, T>(lds, obs_log + (size_t)s0 * n * kObsDim, block_end, i, valid, o);
    const int par = k & 1;
    red_cause[par][tid] = cause;
    red_term[par][tid] = term;
    __syncthreads();
    if (valid) {
      const int b = tid - d;
      int causes = 0;
      T sum = T(0);
      for (int j = 0; j < D; ++j) {                          // drone order d = 0 .. D-1
        causes |= red_cause[par][b + j];
        sum += red_term[par][b + j];
      }
      ++length;
      const int flags = episode_flags(rule, causes, length);
      const T reward = episode_reward(rule, sum, flags);
      ret += reward;
      if (d == 0) {
        if (reward_log != nullptr) reward_log[(size_t)s0 * E + e] = reward;
        if (flags_log != nullptr) flags_log[(size_t)s0 * E + e] = flags;
      }
      if (flags & (kEpTerminated | kEpTruncated)) {
        ++count;
        sum_return += ret;
        sum_length += length;
        length = 0;
        ret = T(0);
        load_state<S, T>(image, ld, i, s);                   // the library's reset, bit for bit (k_reset wrote the image)
        for (int j = 0; j < 4; ++j) prev[j] = clipped[j] = T(0);
      }
    }
    a0 = a0 + 1 == n_sets ? 0 : a0 + 1;
    s0 = s0 + 1 == n_slots ? 0 : s0 + 1;
  }
  if (obs_now != nullptr) {                                  // the current observation: after the resets
    T o[kObsDim];
    if (valid) pack_obs(s, org, clipped, o);
    write_obs_rows<S, T>(lds, obs_now, block_end, i, valid, o);
  }
  if (valid) {
    store_state<S, T>(state, ld, i, s);
    store_last_rpm<DRAG>(last_rpm, ld, i, clipped);
    if (d == 0) {
      cnt.length[e] = length; cnt.ret[e] = ret;
      cnt.count[e] = count; cnt.sum_return[e] = sum_return; cnt.sum_length[e] = sum_length;
    }
  }
}

}  // namespace mds
