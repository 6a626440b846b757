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
//
// k_rollout_episodes_safe is k_rollout_episodes with the collision causes of mds_set_episode_safety (bits 6 and 7, the env's smallest
// h).  The drones of an env already share a workgroup, so the pairwise test is one more exchange through LDS: positions out, barrier,
// the D - 1 env-mates read back.  That makes two barriers per step and lets every exchanged array stay single-buffered (the argument
// stands in the kernel).  LDS of the sibling: observation staging + 5 words (cause, term, h) + 3 position and 3 origin words per lane
// = 58 368 B in float64, 29 696 B in float32, 19 456 B with fp16 storage.
//
// Shared and written out.  The two kernels here, k_rollout_episodes_policy (mds_episode_policy_kernels.hip) and
// k_rollout_episodes_sampled (mds_episode_sample_kernels.hip) share the lane map
// (EpisodeLane) and the type of the env's counters (mds_episode.hpp EpisodeTally); the env's step is stated for the host in
// mds_episode.hpp episode_env_step, and each kernel's loop writes the same lines out.  Why: these kernels keep the instruction order
// they had, the only one measured to be as fast, and any function over the tally or the counters changes it, as does one body under
// a SAFE flag (profiles/asm_equiv_episode_pieces.md, asm_equiv_episode_safety.md).  A change to one loop is a change to all four.
#include "mds_episode.hpp"
#include "mds_episode_random.hpp"

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

// Randomised starts (mds_set_episode_randomisation; the draw: mds_episode_random.hpp).  What the randomised forms of the two rollout
// kernels take besides: the set, and the drones' initial Euler angles (double [n,3]: the handle's init_pose).
template <typename T> struct EpisodeRandomArgs {
  EpisodeRandom<T> set;
  const double* rpy0;
};
// s: the image's state of drone i, just loaded -> the start drawn for the episode of its env that follows `count` completed ones
template <typename S, typename T>
__device__ __forceinline__ void episode_random_reset(const EpisodeRandomArgs<T>& a, int i, int count, State<T>& s) {
  episode_random_start<S, T>(a.set, a.set.first + (uint32_t)i, (uint32_t)count, a.rpy0 + 3 * (size_t)i, s);
}

// mds_reset_episodes: every drone to the start drawn for its env's current `count`, zero RPM echo, and (obs != NULL) its observation
// row.  Flat mapping: it keeps no per-env value, and the draw does not depend on the mapping.
template <typename T, typename S>
__global__ __launch_bounds__(kBlock) void k_episode_reset_random(const int n, const size_t ld, const int D, const EpisodeRandomArgs<T> rnd,
                                                                 const int* __restrict__ count, const S* __restrict__ image,
                                                                 const T* __restrict__ origin, S* __restrict__ state, T* __restrict__ last_rpm,
                                                                 S* __restrict__ obs) {
  __shared__ __align__(16) unsigned char lds[kBlock * kObsDim * sizeof(S)];
  const int i = blockIdx.x * kBlock + threadIdx.x;
  const bool valid = i < n;
  T o[kObsDim];
  if (valid) {
    State<T> s;
    load_state<S, T>(image, ld, i, s);
    episode_random_reset<S, T>(rnd, i, count[i / D], s);
    store_state<S, T>(state, ld, i, s);
    const T rpm[4] = {T(0), T(0), T(0), T(0)};
    for (int k = 0; k < 4; ++k) last_rpm[k * ld + i] = rpm[k];
    if (obs != nullptr) pack_obs(s, load_origin(origin, ld, i), rpm, o);
  }
  if (obs != nullptr) write_obs_rows<S, T>(lds, obs, n, i, valid, o);
}

// Where a thread stands: drone i of the handle, drone d of env e of E (the block's envs start at lane 0, D lanes each); block_end
// bounds the block's rows for write_obs_rows.  (b = tid - d stays in the kernels; the statements keep this order: both for the assembly.)
struct EpisodeLane {
  int tid, i, block_end, d, e, E;
  bool valid;
};
__device__ __forceinline__ EpisodeLane episode_lane(int envs_per_block, int D, int n) {
  EpisodeLane L;
  L.tid = (int)threadIdx.x;
  const int per_block = envs_per_block * D, first = (int)blockIdx.x * per_block;
  L.i = first + L.tid;
  L.block_end = min(first + per_block, n);                  // n = E * D: whole envs
  L.valid = L.tid < per_block && L.i < n;
  const int le = L.tid / D;                                 // env within the block
  L.d = L.tid - le * D;
  L.E = n / D;
  L.e = (int)blockIdx.x * envs_per_block + le;
  return L;
}

// The trailing pack RND is empty -- the kernel of a handle without randomisation, argument for argument what it was before the pack
// existed -- or one EpisodeRandomArgs<T>: the reset arm then moves the image's state by the draw.  The arm runs only in waves where a
// lane is done (the branch is skipped on an empty mask), at a point where the stepped state is dead: the 3 x 40 integer multiplies of
// the three Philox blocks stay off the ordinary step.
template <typename T, typename S, bool RK4, bool DRAG, typename... RND>
__global__ __launch_bounds__(kBlock) void k_rollout_episodes(const Consts<T> c, const EpisodeRule<T> rule, const int n, const size_t ld, const int D,
                                                             const int envs_per_block, S* __restrict__ state, const S* __restrict__ image,
                                                             const T* __restrict__ origin, const T* __restrict__ target, T* __restrict__ last_rpm,
                                                             const S* __restrict__ actions, int a0, const int n_sets, S* __restrict__ obs_log,
                                                             T* __restrict__ reward_log, int* __restrict__ flags_log, int s0, const int n_slots,
                                                             const int n_steps, S* __restrict__ obs_now, const EpisodeCounters<T> cnt,
                                                             const RND... rnd) {
  __shared__ __align__(16) unsigned char lds[kBlock * kObsDim * sizeof(S)];
  __shared__ int red_cause[2][kBlock];
  __shared__ T red_term[2][kBlock];
  const EpisodeLane L = episode_lane(envs_per_block, D, n);
  State<T> s;
  Resid<T> r;
  resid_zero(r);
  V3<T> org = {T(0), T(0), T(0)}, home = org, tgt = org;
  T prev[4] = {T(0), T(0), T(0), T(0)}, clipped[4] = {T(0), T(0), T(0), T(0)};
  EpisodeTally<T> t = {0, 0, 0, T(0), T(0)};
  if (L.valid) {
    load_state<S, T>(state, ld, L.i, s);
    org = load_origin(origin, ld, L.i);
    home = {(T)image[sidx(0, L.i, ld)], (T)image[sidx(1, L.i, ld)], (T)image[sidx(2, L.i, ld)]};
    tgt = load_origin(target, ld, L.i);       // (held across the loop: reloading both per step frees no register and measured no faster)
    if (DRAG)
      for (int k = 0; k < 4; ++k) prev[k] = last_rpm[k * ld + L.i];
    t.length = cnt.length[L.e]; t.ret = cnt.ret[L.e];
    t.count = cnt.count[L.e]; t.sum_return = cnt.sum_return[L.e]; t.sum_length = cnt.sum_length[L.e];
  }
  for (int k = 0; k < n_steps; ++k) {
    T o[kObsDim];
    int cause = 0;
    T term = T(0);
    if (L.valid) {
      T act[4];
      load4<S, T>(actions + ((size_t)a0 * n + L.i) * 4, act);
      aviary_step_any<T, RK4, DRAG, false>(c, s, r, act, prev, clipped);
      if (obs_log != nullptr) pack_obs(s, org, clipped, o);
      cause = episode_causes(rule, s, s.p.z + org.z, home);
      term = episode_reward_term(rule, s.p, tgt);
    }
    // the logged row is the transition's result: before any reset
    if (obs_log != nullptr) write_obs_rows<S, T>(lds, obs_log + (size_t)s0 * n * kObsDim, L.block_end, L.i, L.valid, o);
    const int par = k & 1;
    red_cause[par][L.tid] = cause;
    red_term[par][L.tid] = term;
    __syncthreads();
    if (L.valid) {
      const int b = L.tid - L.d;
      int causes = 0;
      T sum = T(0);
      for (int j = 0; j < D; ++j) {                          // drone order d = 0 .. D-1
        causes |= red_cause[par][b + j];
        sum += red_term[par][b + j];
      }
      ++t.length;
      const int flags = episode_flags(rule, causes, t.length);
      const T reward = episode_reward(rule, sum, flags);
      t.ret += reward;
      if (L.d == 0) {
        if (reward_log != nullptr) reward_log[(size_t)s0 * L.E + L.e] = reward;
        if (flags_log != nullptr) flags_log[(size_t)s0 * L.E + L.e] = flags;
      }
      if (flags & (kEpTerminated | kEpTruncated)) {
        ++t.count;
        t.sum_return += t.ret;
        t.sum_length += t.length;
        t.length = 0;
        t.ret = T(0);
        load_state<S, T>(image, ld, L.i, s);                   // the library's reset, bit for bit (k_reset wrote the image)
        if constexpr (sizeof...(RND) != 0) episode_random_reset<S, T>(rnd..., L.i, t.count, s);      // ... moved by the episode's draw
        for (int j = 0; j < 4; ++j) prev[j] = clipped[j] = T(0);
      }
    }
    a0 = a0 + 1 == n_sets ? 0 : a0 + 1;
    s0 = s0 + 1 == n_slots ? 0 : s0 + 1;
  }
  if (obs_now != nullptr) {                                  // the current observation: after the resets
    T o[kObsDim];
    if (L.valid) pack_obs(s, org, clipped, o);
    write_obs_rows<S, T>(lds, obs_now, L.block_end, L.i, L.valid, o);
  }
  if (L.valid) {
    store_state<S, T>(state, ld, L.i, s);
    store_last_rpm<DRAG>(last_rpm, ld, L.i, clipped);
    if (L.d == 0) {
      cnt.length[L.e] = t.length; cnt.ret[L.e] = t.ret;
      cnt.count[L.e] = t.count; cnt.sum_return[L.e] = t.sum_return; cnt.sum_length[L.e] = t.sum_length;
    }
  }
}

// p[0 .. n) = +inf: h_min_step / h_min_episode of an env with nothing tested yet
template <typename T> __global__ void k_episode_fill_inf(const int n, T* __restrict__ p) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = T(INFINITY);
}

// what the sibling kernel takes besides: the set, and the two per-env outputs [E] (mds_episode_safety_ptrs)
template <typename T> struct EpisodeSafetyArgs {
  EpisodeSafety<T> set;
  T* h_min_step;
  T* h_min_episode;
};

// One lane's tests of a step: its stepped position against the D - 1 env-mates' (lanes b .. b + D - 1 of the position and origin arrays
// in LDS) and against the obstacles; the bits into `cause`, the smallest h returned.
template <typename T>
__device__ __forceinline__ T episode_safety_lane(const EpisodeSafety<T>& set, const T* pos_x, const T* pos_y, const T* pos_z, const T* org_x,
                                                 const T* org_y, const T* org_z, int b, int d, int D, V3<T> p, V3<T> org, int& cause) {
  T h_lane = T(INFINITY);
  for (int j = 0; j < D; ++j) {
    if (j == d) continue;
    // local parts and origin parts differenced separately (env_substep's downwash does the same): a far origin keeps the resolution
    const T ex = (pos_x[b + j] - p.x) + (org_x[b + j] - org.x);
    const T ey = (pos_y[b + j] - p.y) + (org_y[b + j] - org.y);
    const T ez = (pos_z[b + j] - p.z) + (org_z[b + j] - org.z);
    episode_safety_test(episode_barrier(ex, ey, ez, set.inv_zscale, set.neg_ds4_pair), kEpCausePair, cause, h_lane);
  }
  for (int m = 0; m < set.n_obs; ++m) {                      // (wave-uniform rows of the argument block)
    const T ex = p.x - (set.obs[m][0] - org.x);
    const T ey = p.y - (set.obs[m][1] - org.y);
    const T ez = p.z - (set.obs[m][2] - org.z);
    episode_safety_test(episode_barrier(ex, ey, ez, set.inv_zscale, set.obs[m][3]), kEpCauseObstacle, cause, h_lane);
  }
  return h_lane;
}

template <typename T, typename S, bool RK4, bool DRAG, typename... RND>
__global__ __launch_bounds__(kBlock) void k_rollout_episodes_safe(const Consts<T> c, const EpisodeRule<T> rule, const int n, const size_t ld,
                                                                  const int D, const int envs_per_block, S* __restrict__ state,
                                                                  const S* __restrict__ image, const T* __restrict__ origin,
                                                                  const T* __restrict__ target, T* __restrict__ last_rpm,
                                                                  const S* __restrict__ actions, int a0, const int n_sets, S* __restrict__ obs_log,
                                                                  T* __restrict__ reward_log, int* __restrict__ flags_log, int s0, const int n_slots,
                                                                  const int n_steps, S* __restrict__ obs_now, const EpisodeCounters<T> cnt,
                                                                  const EpisodeSafetyArgs<T> safe, const RND... rnd) {
  __shared__ __align__(16) unsigned char lds[kBlock * kObsDim * sizeof(S)];
  __shared__ int red_cause[kBlock];
  __shared__ T red_term[kBlock], red_h[kBlock];
  __shared__ T pos_x[kBlock], pos_y[kBlock], pos_z[kBlock], org_x[kBlock], org_y[kBlock], org_z[kBlock];
  const EpisodeLane L = episode_lane(envs_per_block, D, n);
  const int b = L.tid - L.d;                                // the env's first lane: lanes b .. b + D - 1 are its drones, valid when this one is
  State<T> s;
  Resid<T> r;
  resid_zero(r);
  V3<T> org = {T(0), T(0), T(0)}, home = org, tgt = org;
  T prev[4] = {T(0), T(0), T(0), T(0)}, clipped[4] = {T(0), T(0), T(0), T(0)};
  EpisodeTally<T> t = {0, 0, 0, T(0), T(0)};
  T h_step = T(INFINITY), h_episode = T(INFINITY);          // the env's smallest h of the last step, and of its running episode
  if (L.valid) {
    load_state<S, T>(state, ld, L.i, s);
    org = load_origin(origin, ld, L.i);
    home = {(T)image[sidx(0, L.i, ld)], (T)image[sidx(1, L.i, ld)], (T)image[sidx(2, L.i, ld)]};
    tgt = load_origin(target, ld, L.i);
    if (DRAG)
      for (int k = 0; k < 4; ++k) prev[k] = last_rpm[k * ld + L.i];
    t.length = cnt.length[L.e]; t.ret = cnt.ret[L.e];
    t.count = cnt.count[L.e]; t.sum_return = cnt.sum_return[L.e]; t.sum_length = cnt.sum_length[L.e];
    h_episode = safe.h_min_episode[L.e];
    org_x[L.tid] = org.x; org_y[L.tid] = org.y; org_z[L.tid] = org.z;   // constant over the launch: staged once, published by barrier A of step 0
  }
  for (int k = 0; k < n_steps; ++k) {
    T o[kObsDim];
    int cause = 0;
    T term = T(0), h_lane = T(INFINITY);
    if (L.valid) {
      T act[4];
      load4<S, T>(actions + ((size_t)a0 * n + L.i) * 4, act);
      aviary_step_any<T, RK4, DRAG, false>(c, s, r, act, prev, clipped);
      if (obs_log != nullptr) pack_obs(s, org, clipped, o);
      cause = episode_causes(rule, s, s.p.z + org.z, home);
      term = episode_reward_term(rule, s.p, tgt);
      pos_x[L.tid] = s.p.x; pos_y[L.tid] = s.p.y; pos_z[L.tid] = s.p.z;           // the stepped, pre-reset local position
    }
    // the logged row is the transition's result: before any reset
    if (obs_log != nullptr) write_obs_rows<S, T>(lds, obs_log + (size_t)s0 * n * kObsDim, L.block_end, L.i, L.valid, o);
    // Two barriers per step.  A: every lane has published its position.  B: every lane has published its cause word, reward term and
    // smallest h.  pos_* is written before A and read between A and B; red_* is written between A and B and read after B.  A wave
    // writes pos_* of step k + 1 only after it has passed B of step k, which every wave reaches after its pos_* reads of step k; it
    // writes red_* of step k + 1 only after A of step k + 1, which every wave reaches after its red_* reads of step k.  So no word is
    // overwritten while a wave one barrier behind still reads it, and no array needs a parity copy.  org_* is written once, before
    // the first A, and only read afterwards.  (write_obs_rows stages within a wave: it takes no part in this.)
    __syncthreads();                                                         // A
    if (L.valid) h_lane = episode_safety_lane(safe.set, pos_x, pos_y, pos_z, org_x, org_y, org_z, b, L.d, D, s.p, org, cause);
    red_cause[L.tid] = cause;
    red_term[L.tid] = term;
    red_h[L.tid] = h_lane;
    __syncthreads();                                                         // B
    if (L.valid) {
      int causes = 0;
      T sum = T(0);
      h_step = T(INFINITY);
      for (int j = 0; j < D; ++j) {                          // drone order d = 0 .. D-1
        causes |= red_cause[b + j];
        sum += red_term[b + j];
        h_step = m_min(red_h[b + j], h_step);
      }
      h_episode = m_min(h_step, h_episode);
      ++t.length;
      const int flags = episode_flags(rule, causes, t.length);
      const T reward = episode_reward(rule, sum, flags);
      t.ret += reward;
      if (L.d == 0) {
        if (reward_log != nullptr) reward_log[(size_t)s0 * L.E + L.e] = reward;
        if (flags_log != nullptr) flags_log[(size_t)s0 * L.E + L.e] = flags;
      }
      if (flags & (kEpTerminated | kEpTruncated)) {
        ++t.count;
        t.sum_return += t.ret;
        t.sum_length += t.length;
        t.length = 0;
        t.ret = T(0);
        h_episode = T(INFINITY);
        load_state<S, T>(image, ld, L.i, s);                   // the library's reset, bit for bit (k_reset wrote the image)
        if constexpr (sizeof...(RND) != 0) episode_random_reset<S, T>(rnd..., L.i, t.count, s);      // ... moved by the episode's draw
        for (int j = 0; j < 4; ++j) prev[j] = clipped[j] = T(0);
      }
    }
    a0 = a0 + 1 == n_sets ? 0 : a0 + 1;
    s0 = s0 + 1 == n_slots ? 0 : s0 + 1;
  }
  if (obs_now != nullptr) {                                  // the current observation: after the resets
    T o[kObsDim];
    if (L.valid) pack_obs(s, org, clipped, o);
    write_obs_rows<S, T>(lds, obs_now, L.block_end, L.i, L.valid, o);
  }
  if (L.valid) {
    store_state<S, T>(state, ld, L.i, s);
    store_last_rpm<DRAG>(last_rpm, ld, L.i, clipped);
    if (L.d == 0) {
      cnt.length[L.e] = t.length; cnt.ret[L.e] = t.ret;
      cnt.count[L.e] = t.count; cnt.sum_return[L.e] = t.sum_return; cnt.sum_length[L.e] = t.sum_length;
      if (n_steps > 0) safe.h_min_step[L.e] = h_step;
      safe.h_min_episode[L.e] = h_episode;
    }
  }
}

}  // namespace mds
