// An MLP policy inside the episode rollout kernel (include/mds.h mds_rollout_episodes_policy; the arithmetic: mds_policy.hpp).
//
// k_rollout_episodes_policy is k_rollout_episodes_safe (mds_episode_kernels.hip: the same lane map and tally, the same two barriers per
// step and single-buffered exchange arrays, the loop written out here as there and for the reason given there) with the read of the
// action table replaced by the policy: at the top of every step a lane forms the 12 features of its drone from the state it holds --
// the post-reset state where its env was just done, the loaded state at the first step of a launch -- evaluates the network and
// commands the resulting RPM, which goes through aviary_step_any like a table action and, where a ring is given, into the action log.
// The collision causes and the randomised starts are run-time flags here, not sibling kernels (wave-uniform branches): with the
// collision causes off barrier A still runs and the position exchange does not.
//
// Weights.  They are the same for every lane, so they are wave-uniform operands.  Route taken: scalar loads.  The handle keeps the
// padded weights in device memory that nothing writes while a launch reads it; the kernels read them through a constant-address-space
// pointer with indices that are uniform over the wave, which the compiler turns into s_load_dwordx4/x8/x16 batches into SGPRs, and
// every FMA takes its weight as its one scalar operand.  No LDS (the observation staging and the safety exchange keep all of theirs),
// no vector memory instruction and no VGPR per weight.  The alternative, a broadcast ds_read_b128 per four weights, would put one LDS
// instruction beside every four FMAs of all four SIMDs of a CU through the one LDS pipe, and 20 KB (float64: 40 KB) beside the 58 KB
// the float64 kernel already holds.
//
// Registers.  The first hidden layer (W values) stays in registers under compile-time indices: W is a template argument, one of
// kPolicyWidths.  The second hidden layer is never held (policy_eval_w).  0 bytes of scratch in every instantiation
// (tests/test_episode_policy_cpu.py asserts it from the compiler's resource figures).
#include "mds_policy.hpp"

namespace mds {

// the policy as the kernels take it: the weights padded to the instantiated width, in T, in device memory
template <typename T> struct EpisodePolicy {
  const T* w;
  int n_hidden, activation;
  T rpm_base, rpm_scale;
};

// the weights as the evaluation reads them: constant address space on the device (uniform index -> scalar load)
#if defined(__HIP_DEVICE_COMPILE__)
template <typename T> using PolicyWeights = const __attribute__((address_space(4))) T*;
#else
template <typename T> using PolicyWeights = const T*;
#endif
template <typename T> __device__ __forceinline__ PolicyWeights<T> policy_weights(const EpisodePolicy<T>& pol) { return (PolicyWeights<T>)pol.w; }

// A by-value argument block, word by word through scalar registers the optimiser cannot look into.  Why: the rollout kernel keeps far
// more wave-uniform values alive across its step loop than there are scalar registers, and the register allocator parks the excess in
// lanes of a vector register.  A value it knows to be an invariant load from the argument segment it prefers to load again -- after it
// has already set a stack slot aside for it, which then stays in the kernel's private segment (36 or 100 bytes, never accessed, but
// scratch is set up for every wave).  Values that come out of here are not such loads: they are parked in lanes, and the private
// segment is 0 bytes.
template <typename X> __device__ __forceinline__ X uniform_copy(const X& x) {
  static_assert(sizeof(X) % 4 == 0, "whole words");
  constexpr int N = (int)(sizeof(X) / 4);
  unsigned w[N];
  __builtin_memcpy(w, &x, sizeof(X));
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
  for (int k = 0; k < N; ++k) asm volatile("" : "+s"(w[k]));
#endif
  X y;
  __builtin_memcpy(&y, w, sizeof(X));
  return y;
}

// features x -> the commanded RPM
template <typename T, int W> __device__ __forceinline__ void episode_policy_act(const EpisodePolicy<T>& pol, const T x[kPolicyIn], T rpm[4]) {
  T y[kPolicyOut];
  policy_eval_w<T, W>(policy_weights(pol), pol.n_hidden, pol.activation, x, y);
  policy_rpm(y, pol.rpm_base, pol.rpm_scale, rpm);
}

// mds_episode_policy_compute: the policy on caller-supplied observation rows, flat mapping.  The position feature is
// obs[0:3] - (target_local + origin): both in the world frame.
template <typename T, typename S, int W>
__global__ __launch_bounds__(kBlock) void k_episode_policy_compute(const int n, const size_t ld, const T* __restrict__ origin, const T* __restrict__ target,
                                                                   const EpisodePolicy<T> pol, const S* __restrict__ obs, S* __restrict__ rpm_out) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  T o[kObsDim];
  for (int k = 0; k < 16; ++k) o[k] = (T)obs[(size_t)i * kObsDim + k];
  const V3<T> org = load_origin(origin, ld, i), tl = load_origin(target, ld, i);
  T x[kPolicyIn], rpm[4];
  policy_features_obs(o, V3<T>{tl.x + org.x, tl.y + org.y, tl.z + org.z}, x);
  episode_policy_act<T, W>(pol, x, rpm);
  store4<S, T>(rpm_out + (size_t)i * 4, rpm);
}

template <typename T, typename S, bool RK4, bool DRAG, int W>
__global__ __launch_bounds__(kBlock) void k_rollout_episodes_policy(const Consts<T> c_arg, const EpisodeRule<T> rule_arg, const int n_arg,
                                                                    const size_t ld_arg, const int D_arg, const int envs_per_block_arg,
                                                                    S* __restrict__ state, const S* __restrict__ image,
                                                                    const T* __restrict__ origin, const T* __restrict__ target,
                                                                    T* __restrict__ last_rpm, const EpisodePolicy<T> pol_arg,
                                                                    S* __restrict__ action_log, S* __restrict__ obs_log,
                                                                    T* __restrict__ reward_log, int* __restrict__ flags_log, int s0,
                                                                    const int n_slots_arg, const int n_steps_arg, S* __restrict__ obs_now,
                                                                    const EpisodeCounters<T> cnt_arg, const int safe_on_arg,
                                                                    const EpisodeSafetyArgs<T> safe, const int random_on_arg,
                                                                    const EpisodeRandomArgs<T> rnd_arg) {
  // (uniform_copy says why; `safe` stays in the argument segment: its obstacle rows are indexed at run time)
  const Consts<T> c = uniform_copy(c_arg);
  const EpisodeRule<T> rule = uniform_copy(rule_arg);
  const EpisodePolicy<T> pol = uniform_copy(pol_arg);
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
    if (L.valid) {
      // the policy acts on the state the lane holds: the features are the columns pack_obs would form of it
      T x[kPolicyIn], act[4];
      {
        const Frame<T> F = make_frame(s.q, s.w);
        policy_features(s.p, tgt, rpy_from_rot(F.R, s.q), s.v, F.av, x);
      }
      episode_policy_act<T, W>(pol, x, act);
      if (action_log != nullptr) store4<S, T>(action_log + ((size_t)s0 * n + L.i) * 4, act);
      aviary_step_any<T, RK4, DRAG, false>(c, s, r, act, prev, clipped);
      if (obs_log != nullptr) pack_obs(s, org, clipped, o);
      cause = episode_causes(rule, s, s.p.z + org.z, home);
      term = episode_reward_term(rule, s.p, tgt);
      if (safe_on) {
        pos_x[L.tid] = s.p.x; pos_y[L.tid] = s.p.y; pos_z[L.tid] = s.p.z;         // the stepped, pre-reset local position
      }
    }
    // the logged row is the transition's result: before any reset
    if (obs_log != nullptr) write_obs_rows<S, T>(lds, obs_log + (size_t)s0 * n * kObsDim, L.block_end, L.i, L.valid, o);
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
    store_last_rpm<DRAG>(last_rpm, ld, L.i, clipped);
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
