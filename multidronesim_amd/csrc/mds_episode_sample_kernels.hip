// Gaussian actions drawn inside the episode rollout kernel (include/mds.h mds_rollout_episodes_sampled; the arithmetic:
// mds_policy_noise.hpp).
//
// k_rollout_episodes_sampled is k_rollout_episodes_policy (mds_episode_policy_kernels.hip: the same lane map and tally, the same two
// barriers per step, the loop written out here as there and for the reason given in mds_episode_kernels.hip) with the commanded mean
// replaced by a sample: after the network a lane draws the four normals of its drone from (g, the env's count, the running episode's
// length, epoch), forms a = y + sigma eps and its log-probability, and commands policy_rpm(a).  The Philox block and the Box-Muller
// pair run behind the network, where its first hidden layer is dead: about 40 integer multiplies, two logs, two square roots and two
// sincos per drone-step beside the network's thousands of FMAs.
//
// Three rings more than the sibling: the sample before the clamp, the log-probability, and the rows the action was drawn on.  The last
// is written at the top of the step from the state the lane holds -- pack_obs of it with the current RPM echo, zero after a reset --
// through the observation staging buffer (write_obs_rows stages within a wave: two uses per step need no further barrier).  So that the
// rows of a launch's first step carry the echo of the step before, the kernel reads it from the handle's RPM planes and always leaves it
// there (planes that are not current the entry point fills with NaN before the first launch: what mds_get_obs reports of them).  The
// read is unconditional: under a run-time flag the float64, Euler, no-drag, 32-wide instantiation is left with a never-accessed slot in its private segment.
#include "mds_policy_noise.hpp"

namespace mds {

// y: the network's output -> the sample a, its log-probability, the commanded RPM
template <typename T>
__device__ __forceinline__ T episode_policy_draw(const EpisodePolicy<T>& pol, const PolicyNoise<T>& noise, uint32_t g, int count, int length,
                                                 const T y[4], T a[4], T rpm[4]) {
  T eps[4];
  policy_noise_eps(noise, g, (uint32_t)count, (uint32_t)length, eps);
  const T logp = policy_noise_sample(noise, y, eps, a);
  policy_rpm(a, pol.rpm_base, pol.rpm_scale, rpm);
  return logp;
}

// mds_episode_policy_sample: k_episode_policy_compute plus the draw, at the count and length the handle's counters hold for the env
template <typename T, typename S, int W>
__global__ __launch_bounds__(kBlock) void k_episode_policy_sample(const int n, const size_t ld, const int D, const T* __restrict__ origin,
                                                                  const T* __restrict__ target, const EpisodePolicy<T> pol,
                                                                  const PolicyNoise<T> noise, const int* __restrict__ count,
                                                                  const int* __restrict__ length, const S* __restrict__ obs,
                                                                  S* __restrict__ rpm_out, S* __restrict__ sample_out, T* __restrict__ logp_out) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  T o[kObsDim];
  for (int k = 0; k < 16; ++k) o[k] = (T)obs[(size_t)i * kObsDim + k];
  const V3<T> org = load_origin(origin, ld, i), tl = load_origin(target, ld, i);
  T x[kPolicyIn], y[kPolicyOut], a[4], rpm[4];
  policy_features_obs(o, V3<T>{tl.x + org.x, tl.y + org.y, tl.z + org.z}, x);
  policy_eval_w<T, W>(policy_weights(pol), pol.n_hidden, pol.activation, x, y);
  const int e = i / D;
  const T logp = episode_policy_draw(pol, noise, noise.first + (uint32_t)i, count[e], length[e], y, a, rpm);
  store4<S, T>(rpm_out + (size_t)i * 4, rpm);
  if (sample_out != nullptr) store4<S, T>(sample_out + (size_t)i * 4, a);
  if (logp_out != nullptr) logp_out[i] = logp;
}

// RPM planes that are not current: NaN rather than stale, the value k_get_obs reports of them
template <typename T> __global__ void k_episode_echo_unknown(const size_t count, T* __restrict__ last_rpm) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) last_rpm[i] = (T)__builtin_nanf("");
}

// the rings of the sampled rollout (include/mds.h mds_episode_sample_rings, typed)
template <typename T, typename S> struct EpisodeSampleRings {
  S* acted_obs;
  S* obs;
  S* action;
  S* sample;
  T* logp;
  T* reward;
  int* flags;
};

template <typename T, typename S, bool RK4, bool DRAG, int W>
__global__ __launch_bounds__(kBlock) void k_rollout_episodes_sampled(const Consts<T> c_arg, const EpisodeRule<T> rule_arg, const int n_arg,
                                                                     const size_t ld_arg, const int D_arg, const int envs_per_block_arg,
                                                                     S* __restrict__ state, const S* __restrict__ image,
                                                                     const T* __restrict__ origin, const T* __restrict__ target,
                                                                     T* __restrict__ last_rpm,
                                                                     const EpisodePolicy<T> pol_arg, const PolicyNoise<T> noise_arg,
                                                                     const EpisodeSampleRings<T, S> rings_arg, int s0, const int n_slots_arg,
                                                                     const int n_steps_arg, S* __restrict__ obs_now,
                                                                     const EpisodeCounters<T> cnt_arg, const int safe_on_arg,
                                                                     const EpisodeSafetyArgs<T> safe, const int random_on_arg,
                                                                     const EpisodeRandomArgs<T> rnd_arg) {
  // (uniform_copy says why; `safe` stays in the argument segment: its obstacle rows are indexed at run time)
  const Consts<T> c = uniform_copy(c_arg);
  const EpisodeRule<T> rule = uniform_copy(rule_arg);
  const EpisodePolicy<T> pol = uniform_copy(pol_arg);
  const PolicyNoise<T> noise = uniform_copy(noise_arg);
  const EpisodeSampleRings<T, S> rings = uniform_copy(rings_arg);
  const EpisodeCounters<T> cnt = uniform_copy(cnt_arg);
  const EpisodeRandomArgs<T> rnd = uniform_copy(rnd_arg);
  const int n = uniform_copy(n_arg), D = uniform_copy(D_arg), envs_per_block = uniform_copy(envs_per_block_arg);
  const int n_slots = uniform_copy(n_slots_arg), n_steps = uniform_copy(n_steps_arg);
  const int safe_on = uniform_copy(safe_on_arg), random_on = uniform_copy(random_on_arg);
  const size_t ld = uniform_copy(ld_arg);
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
    // the echo of the step before this launch: what the acted-on rows of step 0 carry
    for (int k = 0; k < 4; ++k) clipped[k] = last_rpm[k * ld + L.i];
    if (DRAG)
      for (int k = 0; k < 4; ++k) prev[k] = last_rpm[k * ld + L.i];
    t.length = cnt.length[L.e]; t.ret = cnt.ret[L.e];
    t.count = cnt.count[L.e]; t.sum_return = cnt.sum_return[L.e]; t.sum_length = cnt.sum_length[L.e];
    if (safe_on) {
      h_episode = safe.h_min_episode[L.e];
      org_x[L.tid] = org.x; org_y[L.tid] = org.y; org_z[L.tid] = org.z;   // constant over the launch: staged once, published by barrier A of step 0
    }
  }
  for (int k = 0; k < n_steps; ++k) {
    T o[kObsDim];
    int cause = 0;
    T term = T(0), h_lane = T(INFINITY);
    // the rows the action of this step is drawn on: what obs_now would have received had the launch ended before this step
    if (rings.acted_obs != nullptr) {
      if (L.valid) pack_obs(s, org, clipped, o);
      write_obs_rows<S, T>(lds, rings.acted_obs + (size_t)s0 * n * kObsDim, L.block_end, L.i, L.valid, o);
    }
    if (L.valid) {
      // the policy acts on the state the lane holds: the features are the columns pack_obs would form of it
      T x[kPolicyIn], y[kPolicyOut], a[4], act[4];
      {
        const Frame<T> F = make_frame(s.q, s.w);
        policy_features(s.p, tgt, rpy_from_rot(F.R, s.q), s.v, F.av, x);
      }
      policy_eval_w<T, W>(policy_weights(pol), pol.n_hidden, pol.activation, x, y);
      const T logp = episode_policy_draw(pol, noise, noise.first + (uint32_t)L.i, t.count, t.length, y, a, act);
      if (rings.sample != nullptr) store4<S, T>(rings.sample + ((size_t)s0 * n + L.i) * 4, a);
      if (rings.logp != nullptr) rings.logp[(size_t)s0 * n + L.i] = logp;
      if (rings.action != nullptr) store4<S, T>(rings.action + ((size_t)s0 * n + L.i) * 4, act);
      aviary_step_any<T, RK4, DRAG, false>(c, s, r, act, prev, clipped);
      if (rings.obs != nullptr) pack_obs(s, org, clipped, o);
      cause = episode_causes(rule, s, s.p.z + org.z, home);
      term = episode_reward_term(rule, s.p, tgt);
      if (safe_on) {
        pos_x[L.tid] = s.p.x; pos_y[L.tid] = s.p.y; pos_z[L.tid] = s.p.z;         // the stepped, pre-reset local position
      }
    }
    // the logged row is the transition's result: before any reset
    if (rings.obs != nullptr) write_obs_rows<S, T>(lds, rings.obs + (size_t)s0 * n * kObsDim, L.block_end, L.i, L.valid, o);
    // Two barriers per step, single-buffered arrays: the argument stands in k_rollout_episodes_safe and does not depend on what is
    // computed between the barriers (with the collision causes off nothing is exchanged between A and B, and red_* keep their order).
    __syncthreads();                                                         // A
    if (safe_on && L.valid) h_lane = episode_safety_lane(safe.set, pos_x, pos_y, pos_z, org_x, org_y, org_z, b, L.d, D, s.p, org, cause);
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
        if (rings.reward != nullptr) rings.reward[(size_t)s0 * L.E + L.e] = reward;
        if (rings.flags != nullptr) rings.flags[(size_t)s0 * L.E + L.e] = flags;
      }
      if (flags & (kEpTerminated | kEpTruncated)) {
        ++t.count;
        t.sum_return += t.ret;
        t.sum_length += t.length;
        t.length = 0;
        t.ret = T(0);
        h_episode = T(INFINITY);
        load_state<S, T>(image, ld, L.i, s);                   // the library's reset, bit for bit (k_reset wrote the image)
        if (random_on) episode_random_reset<S, T>(rnd, L.i, t.count, s);      // ... moved by the episode's draw
        for (int j = 0; j < 4; ++j) prev[j] = clipped[j] = T(0);
      }
    }
    s0 = s0 + 1 == n_slots ? 0 : s0 + 1;
  }
  if (obs_now != nullptr) {                                  // the current observation: after the resets
    T o[kObsDim];
    if (L.valid) pack_obs(s, org, clipped, o);
    write_obs_rows<S, T>(lds, obs_now, L.block_end, L.i, L.valid, o);
  }
  if (L.valid) {
    store_state<S, T>(state, ld, L.i, s);
    store_last_rpm<true>(last_rpm, ld, L.i, clipped);          // (always: the next launch's acted-on rows read it)
    if (L.d == 0) {
      cnt.length[L.e] = t.length; cnt.ret[L.e] = t.ret;
      cnt.count[L.e] = t.count; cnt.sum_return[L.e] = t.sum_return; cnt.sum_length[L.e] = t.sum_length;
      if (safe_on) {
        if (n_steps > 0) safe.h_min_step[L.e] = h_step;
        safe.h_min_episode[L.e] = h_episode;
      }
    }
  }
}

}  // namespace mds
