// Gaussian actions of the MLP policy (include/mds.h mds_set_episode_policy_noise): the draw, the sample and its log-probability -- the
// arithmetic stated once, templated on the compute type T like mds_policy.hpp.  The same header compiles with plain g++
// (tests/episode_sample_main.cpp runs it against the float64 oracle and torch); nothing here is HIP-only, and it calls nothing but
// mds_math.hpp and the Philox of mds_episode_random.hpp.
//
// The distribution is stable-baselines3's DiagGaussianDistribution with a state-independent log_std: a ~ N(y, diag(sigma^2)), y the
// network's output (policy_eval_w), sigma[j] = exp(log_std[j]).
//
// The four standard normals of one drone at one step are a pure function of (seed, g, ordinal, length, epoch):
//   g         first_env * D + i: the drone's index in the whole env set, as for the randomised starts
//   ordinal   the env's count of completed episodes (mds_episode_ptrs ptrs[2], read as uint32) when the action is formed
//   length    the length of the env's running episode at that moment: before the step's increment, 0 for an episode's first step
//   epoch     a per-handle word: 0 after mds_set_episode_policy_noise, + 1 with every host call that restarts every env's running
//             episode (mds_reset, mds_reset_async, mds_reset_episodes, mds_set_episodes with parameters) -- without it a reset that
//             keeps or zeroes `count` would replay the same noise
// so they depend neither on how a rollout is cut into launches, nor on the thread mapping, nor on how the env set is sharded.
//
// Generator: Philox4x32-10 with key = (seed low word, seed high word) of the noise's own seed and counter = (g, ordinal, 3 + length,
// epoch), the sum mod 2^32.  Word 2 starts at 3: even with equal seeds and epoch == generation no block coincides with the three
// blocks b = 0, 1, 2 of a start draw (mds_episode_random.hpp).  One block per drone-step; words (w0, w1) give eps[0], eps[1] and
// (w2, w3) give eps[2], eps[3] by Box-Muller:
//   u     = (2 (w_a >> 9) + 1) 2^-24: an odd integer below 2^24 (exact in fp32, the same quantity in every compute type), never 0 or 1
//   r     = m_sqrt(-2 m_log(u)), at most sqrt(48 ln 2) = 5.77
//   theta = pi * episode_random_unit(w_b), in (-pi, pi): the range m_sincos(float) reduces from
//   eps   = r cos(theta), r sin(theta)
//
// Sample: a[j] = m_fma(sigma[j], eps[j], y[j]); the commanded RPM is policy_rpm(a): the +-1 clamp acts on the sample, as SB3 clips a
// sampled action before the env sees it.
// Log-probability of the UNCLIPPED sample (SB3's convention, Normal(y, sigma).log_prob(a).sum(-1)):
//   logp = -(0.5 * sum_j eps[j]^2) - (sum_j log_std[j] + 2 ln(2 pi))
// the sum of squares one m_fma chain, j ascending from 0; the second parenthesis one host constant, double rounded to T.  It is formed
// from eps, never from (a - y) / sigma: that quotient loses eps where sigma is small against y.
#pragma once
#include "mds_episode_random.hpp"
#include "mds_math.hpp"

namespace mds {

constexpr uint32_t kPolicyNoiseBlock0 = 3;          // counter word 2 of the block of length 0

// the noise as the draw reads it (word-sized: passed to the kernels by value)
template <typename T> struct PolicyNoise {
  uint32_t key[2];          // seed low word, seed high word
  uint32_t first;           // first_env * D: g of this handle's drone 0
  uint32_t epoch;
  T sigma[4];               // exp(log_std), formed in double
  T logp_const;             // sum_j log_std[j] + 2 ln(2 pi), formed in double
};

// the caller's parameters (include/mds.h mds_episode_policy_noise, as plain values) -> the set in T
template <typename T> inline void fill_policy_noise(uint64_t seed, uint32_t first, uint32_t epoch, const double log_std[4], PolicyNoise<T>& p) {
  p.key[0] = (uint32_t)seed;
  p.key[1] = (uint32_t)(seed >> 32);
  p.first = first;
  p.epoch = epoch;
  double sum = 0.0;
  for (int j = 0; j < 4; ++j) {
    p.sigma[j] = (T)exp(log_std[j]);
    sum += log_std[j];
  }
  p.logp_const = (T)(sum + 2.0 * 1.8378770664093454835606594728112353);          // ln(2 pi)
}

// the block of drone g at (ordinal, length, epoch)
MDS_HD void policy_noise_words(const uint32_t key[2], uint32_t g, uint32_t ordinal, uint32_t length, uint32_t epoch, uint32_t word[4]) {
  const uint32_t counter[4] = {g, ordinal, kPolicyNoiseBlock0 + length, epoch};
  philox4x32_10(counter, key, word);
}

// two standard normals of two words
template <typename T> MDS_HD void policy_noise_pair(uint32_t wa, uint32_t wb, T& e0, T& e1) {
  const T u = (T)(int)(2u * (wa >> 9) + 1u) * T(5.9604644775390625e-8);          // 2^-24: exact
  const T r = m_sqrt(T(-2) * m_log(u));
  T s, c;
  m_sincos(T(3.14159265358979323846) * episode_random_unit<T>(wb), &s, &c);
  e0 = r * c;
  e1 = r * s;
}
template <typename T> MDS_HD void policy_noise_box_muller(const uint32_t word[4], T eps[4]) {
  policy_noise_pair<T>(word[0], word[1], eps[0], eps[1]);
  policy_noise_pair<T>(word[2], word[3], eps[2], eps[3]);
}

// eps[4] of drone g at (ordinal, length)
template <typename T> MDS_HD void policy_noise_eps(const PolicyNoise<T>& p, uint32_t g, uint32_t ordinal, uint32_t length, T eps[4]) {
  uint32_t word[4];
  policy_noise_words(p.key, g, ordinal, length, p.epoch, word);
  policy_noise_box_muller<T>(word, eps);
}

// the sample a[4] around the network's output y[4], and its log-probability
template <typename T> MDS_HD T policy_noise_sample(const PolicyNoise<T>& p, const T y[4], const T eps[4], T a[4]) {
  T ss = T(0);
  for (int j = 0; j < 4; ++j) {
    a[j] = m_fma(p.sigma[j], eps[j], y[j]);
    ss = m_fma(eps[j], eps[j], ss);
  }
  return -(T(0.5) * ss) - p.logp_const;
}

}  // namespace mds
