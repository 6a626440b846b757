// Per-env episodes: the termination tests of one drone, the reward term of one drone and the env-level rule, templated on the compute
// type T like mds_math.hpp.  The same header compiles with plain g++ (tests/test_episode_rule_cpu.py runs it over rows of the float64
// oracle); nothing here is HIP-only.
//
// Cause bits of a drone after a control step (on the stepped state, in T):
//   0  a state component is not finite (always on)
//   1  world z < z_min or > z_max
//   2  |p - home|^2 > max_dist^2        home: the drone's reset position as the reset writes it (stored, storage-rounded, local frame)
//   3  1 - 2 (qx^2 + qy^2) < cos(max_tilt)     the body z axis against world z
//   4  |v|^2 > max_speed^2
//   5  |w|^2 > max_rate^2
//   6  an env-mate is inside the pair safety set: h < 0 with Ds = 2 safety_radius      (mds_set_episode_safety; off without it)
//   7  a sphere obstacle is inside the safety set: h < 0 with Ds = safety_radius + r   (the same)
// h is the zeroth-order barrier of the CBF filter (mds_cbf.hpp cbf_row_o2_pairs, [UPSTREAM] cbf/cbf.py custom_hdots):
//   h = (ex^2 + ey^2)^2 + (ez / zscale)^4 - Ds^4,   e the separation.  A NaN h fires neither bit (bit 0 owns states that are not finite).
// A threshold that is not finite or out of range switches its test off: fill_episode_rule turns it into a bound no finite value
// crosses (and a value that is not finite is bit 0's).
// Env: terminated = OR over its drones; truncated = !terminated and the episode has run max_steps control steps (0: never);
// done = terminated | truncated puts every drone of the env back.  Reward of the transition:
//   sum over d = 0 .. D-1 (in this order, in T) of max(0, r0 - |p_d - target_d|^4)  -  (terminated ? term_penalty : 0)
// ([UPSTREAM] HoverAviary._computeReward's form, r0 = 2 there).
#pragma once
#include "mds_math.hpp"

namespace mds {

constexpr int kEpTerminated = 1, kEpTruncated = 2, kEpCauseShift = 8;     // the flags word: bit 0, bit 1, cause bits at 8..15
constexpr int kEpCauses = 8;
constexpr int kEpCausePair = 1 << 6, kEpCauseObstacle = 1 << 7;
constexpr int kEpMaxObstacles = 16;

// the thresholds as the tests read them (word-sized: passed to the kernels by value)
template <typename T> struct EpisodeRule {
  T z_min, z_max, max_dist2, cos_tilt, max_speed2, max_rate2, r0, term_penalty;
  int max_steps, pad;
};

// the caller's parameters (include/mds.h mds_episode_params, as plain doubles) -> the rule in T
template <typename T>
inline void fill_episode_rule(int max_steps, double z_min, double z_max, double max_dist, double max_tilt, double max_speed, double max_rate,
                              double r0, double term_penalty, EpisodeRule<T>& r) {
  const double inf = (double)INFINITY;
  auto square_or_off = [&](double x) { return (x > 0.0 && x < inf) ? x * x : inf; };
  r.z_min = (T)((z_min > -inf && z_min < inf) ? z_min : -inf);
  r.z_max = (T)((z_max > -inf && z_max < inf) ? z_max : inf);
  r.max_dist2 = (T)square_or_off(max_dist);
  r.cos_tilt = (T)((max_tilt > 0.0 && max_tilt < 3.14159265358979323846) ? cos(max_tilt) : -inf);
  r.max_speed2 = (T)square_or_off(max_speed);
  r.max_rate2 = (T)square_or_off(max_rate);
  r.r0 = (T)r0;
  r.term_penalty = (T)term_penalty;
  r.max_steps = max_steps > 0 ? max_steps : 0;
  r.pad = 0;
}

// the safety set as the tests read it (passed to the kernel by value: the obstacle rows are wave-uniform reads of the argument block)
template <typename T> struct EpisodeSafety {
  T inv_zscale, neg_ds4_pair;
  int n_obs, pad;
  T obs[kEpMaxObstacles][4];          // centre x, y, z (world frame), -(safety_radius + radius)^4
};

// -Ds^4 the way mds_cbf.hpp cbf_neg_ds4 forms it
template <typename T> inline T episode_neg_ds4(T Ds) {
  const T Ds2 = Ds * Ds;
  return -(Ds2 * Ds2);
}

// the caller's parameters (include/mds.h mds_episode_safety; obstacles [n_obs,4] = centre xyz, radius) -> the set in T
template <typename T> inline void fill_episode_safety(double safety_radius, double zscale, int n_obs, const double* obstacles, EpisodeSafety<T>& s) {
  s.inv_zscale = (T)(1.0 / zscale);
  s.neg_ds4_pair = episode_neg_ds4((T)(2.0 * safety_radius));
  s.n_obs = n_obs;
  s.pad = 0;
  for (int k = 0; k < kEpMaxObstacles; ++k) {
    const bool on = k < n_obs;
    for (int c = 0; c < 3; ++c) s.obs[k][c] = on ? (T)obstacles[4 * k + c] : T(0);
    s.obs[k][3] = on ? episode_neg_ds4((T)safety_radius + (T)obstacles[4 * k + 3]) : T(0);
  }
}

// h of one separation, in the operation order of the h lines of cbf_row_o2_pairs (no contraction of s)
template <typename T> MDS_HD T episode_barrier(T ex, T ey, T ez, T inv_zscale, T neg_ds4) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const T ex2 = ex * ex, ey2 = ey * ey;
  const T s = ex2 + ey2;
  const T ezc = ez * inv_zscale;
  const T ezc2 = ezc * ezc;
  T h = m_fma(ezc2, ezc2, neg_ds4);
  h = m_fma(s, s, h);
  return h;
}

// one tested separation: its cause bit into `cause` when h < 0, and h into the running minimum (a NaN h does neither)
template <typename T> MDS_HD void episode_safety_test(T h, int bit, int& cause, T& h_min) {
  cause |= (h < T(0)) ? bit : 0;
  h_min = (h < h_min) ? h : h_min;
}

// the cause bits of one drone.  p: position in the frame `home` is given in; world_z: the same drone's world height
template <typename T> MDS_HD int episode_causes(const EpisodeRule<T>& r, const State<T>& s, T world_z, V3<T> home) {
  // x * 0 is 0 for a finite x and NaN otherwise: one accumulation over the 13 components
  T f = s.p.x * T(0);
  f = m_fma(s.p.y, T(0), f); f = m_fma(s.p.z, T(0), f);
  for (int k = 0; k < 4; ++k) f = m_fma(s.q[k], T(0), f);
  f = m_fma(s.v.x, T(0), f); f = m_fma(s.v.y, T(0), f); f = m_fma(s.v.z, T(0), f);
  f = m_fma(s.w.x, T(0), f); f = m_fma(s.w.y, T(0), f); f = m_fma(s.w.z, T(0), f);
  const V3<T> d = s.p - home;
  int c = (f == T(0)) ? 0 : 1;
  c |= (world_z < r.z_min || world_z > r.z_max) ? 2 : 0;
  c |= (dot(d, d) > r.max_dist2) ? 4 : 0;
  c |= (T(1) - T(2) * m_fma(s.q[0], s.q[0], s.q[1] * s.q[1]) < r.cos_tilt) ? 8 : 0;
  c |= (dot(s.v, s.v) > r.max_speed2) ? 16 : 0;
  c |= (dot(s.w, s.w) > r.max_rate2) ? 32 : 0;
  return c;
}

// one drone's term of the reward: max(0, r0 - |p - target|^4), p and target in the same frame.  A NaN distance gives 0.
template <typename T> MDS_HD T episode_reward_term(const EpisodeRule<T>& r, V3<T> p, V3<T> target) {
  const V3<T> e = p - target;
  const T d2 = dot(e, e);
  const T v = r.r0 - d2 * d2;
  return v > T(0) ? v : T(0);
}

// the env's flags word from the OR of its drones' cause bits and the length the episode has reached with this step
template <typename T> MDS_HD int episode_flags(const EpisodeRule<T>& r, int causes, int length) {
  const bool term = causes != 0;
  const bool trunc = !term && r.max_steps > 0 && length >= r.max_steps;
  return (term ? kEpTerminated : 0) | (trunc ? kEpTruncated : 0) | (causes << kEpCauseShift);
}
// the env's reward from the sum of its drones' terms
template <typename T> MDS_HD T episode_reward(const EpisodeRule<T>& r, T sum_terms, int flags) {
  return (flags & kEpTerminated) ? sum_terms - r.term_penalty : sum_terms;
}

// an env's counters as its step carries them: the running episode's length and return, and of the completed episodes their number,
// summed returns, summed lengths.  (A plain aggregate on purpose: with default member initialisers the rollout kernels that hold one
// come out in another instruction order.)
template <typename T> struct EpisodeTally {
  int length, count, sum_length;
  T ret, sum_return;
};
// what a step of the env hands back
template <typename T> struct EpisodeStep {
  int flags;
  T reward;
  bool done;
};
// One control step of an env, from the OR of its drones' cause bits and the sum of their reward terms: the episode grows by the step,
// flags and reward follow from the rule, and a done episode (terminated or truncated) goes into the completed ones and leaves a fresh
// tally.  The statement of the env's step for the host (tests/test_episode_cpu.py carries it over steps and envs against the oracle's
// counter lines).  The three rollout kernels write these lines out in their loops, with the log stores between `ret += reward` and the
// done part (mds_episode_kernels.hip says why); they are to be kept equal to this function.
template <typename T> MDS_HD EpisodeStep<T> episode_env_step(const EpisodeRule<T>& r, int causes, T sum_terms, EpisodeTally<T>& t) {
  ++t.length;
  const int flags = episode_flags(r, causes, t.length);
  const T reward = episode_reward(r, sum_terms, flags);
  t.ret += reward;
  const bool done = (flags & (kEpTerminated | kEpTruncated)) != 0;
  if (done) {
    ++t.count;
    t.sum_return += t.ret;
    t.sum_length += t.length;
    t.length = 0;
    t.ret = T(0);
  }
  return {flags, reward, done};
}

}  // namespace mds
