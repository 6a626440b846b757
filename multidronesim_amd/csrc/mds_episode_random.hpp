// Randomised episode starts: a counter-based generator and the start state drawn from it, templated on the compute type T like
// mds_episode.hpp.  The same header compiles with plain g++ (tests/test_episode_random_cpu.py runs it against a NumPy restatement);
// nothing here is HIP-only.
//
// The start state of a drone is a pure function of (seed, g, ordinal, generation):
//   g            first_env * D + i: the drone's index in the whole env set (first_env: the global index of this handle's env 0)
//   ordinal      the env's count of completed episodes (mds_episode_ptrs, read as uint32); in-kernel the value after the increment for
//                the episode that just ended
//   generation   a per-handle word: 0 after mds_set_episode_randomisation, + 1 with every mds_reset_episodes
// so it depends neither on how a rollout is cut into launches, nor on the thread mapping, nor on how the env set is sharded.
//
// Generator: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123's known answers are in
// tests/test_episode_random_cpu.py).  key = (seed low word, seed high word); counter = (g, ordinal, b, generation) for block b = 0, 1, 2.
// The twelve words of blocks 0..2, in order: position x y z | roll pitch yaw | world velocity x y z | body rates x y z.
//
// Word x -> offset: k = 2 (x >> 8) + 1 - 2^24, an odd integer with |k| < 2^24 (exact in fp32); s = k 2^-24 in (-1, 1), symmetric, never 0
// or +-1, the same 24-bit quantity in every compute type; offset = s * (T)half_width, and exactly +0 for a half-width of 0.
//
// Start: position = the reset image's + offset (local frame); attitude = quat_from_euler<T>((T)rpy0 + offset), rpy0 the double poses of
// the last mds_reset -- the image's own quaternion, bit for bit, when the three attitude half-widths are 0; velocity and body rates =
// their offsets.  Every component goes through the storage type S, (T)(S)v, before it is used: a randomised start is a state that could
// have been stored, as the image's is.  With all half-widths 0 the start is the image.
#pragma once
#include "mds_math.hpp"

namespace mds {

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;      // the round's multipliers
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;      // the key's increments

// 32 x 32 -> 64 in two halves: v_mul_hi_u32 and v_mul_lo_u32 on the device, one uint64_t product on the host
MDS_HD void philox_mul(uint32_t a, uint32_t b, uint32_t& hi, uint32_t& lo) {
#if defined(__HIP_DEVICE_COMPILE__)
  hi = __umulhi(a, b);
  lo = a * b;
#else
  const uint64_t p = (uint64_t)a * (uint64_t)b;
  hi = (uint32_t)(p >> 32);
  lo = (uint32_t)p;
#endif
}

// out = Philox4x32-10(counter, key)
MDS_HD void philox4x32_10(const uint32_t counter[4], const uint32_t key[2], uint32_t out[4]) {
  uint32_t c0 = counter[0], c1 = counter[1], c2 = counter[2], c3 = counter[3], k0 = key[0], k1 = key[1];
  for (int round = 0; round < 10; ++round) {
    uint32_t hi0, lo0, hi1, lo1;
    philox_mul(kPhiloxM0, c0, hi0, lo0);
    philox_mul(kPhiloxM1, c2, hi1, lo1);
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += kPhiloxW0;
    k1 += kPhiloxW1;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// s of one word
template <typename T> MDS_HD T episode_random_unit(uint32_t x) {
  const int k = 2 * (int)(x >> 8) + 1 - (1 << 24);
  return (T)k * T(5.9604644775390625e-8);                  // 2^-24: exact
}

// the randomisation as the draw reads it (word-sized: passed to the kernels by value)
template <typename T> struct EpisodeRandom {
  uint32_t key[2];          // seed low word, seed high word
  uint32_t first;           // first_env * D: g of this handle's drone 0
  uint32_t generation;
  T half[12];               // half-widths: position 3 | roll pitch yaw | world velocity 3 | body rates 3
};

// the caller's parameters (include/mds.h mds_episode_randomisation, as plain doubles) -> the set in T
template <typename T>
inline void fill_episode_random(uint64_t seed, uint32_t first, uint32_t generation, const double pos[3], const double rpy[3],
                                const double vel[3], const double rate[3], EpisodeRandom<T>& r) {
  r.key[0] = (uint32_t)seed;
  r.key[1] = (uint32_t)(seed >> 32);
  r.first = first;
  r.generation = generation;
  for (int k = 0; k < 3; ++k) {
    r.half[k] = (T)pos[k];
    r.half[3 + k] = (T)rpy[k];
    r.half[6 + k] = (T)vel[k];
    r.half[9 + k] = (T)rate[k];
  }
}

// the twelve offsets of drone g in the episode `ordinal` of its env.  The product is rounded on its own (no contraction into the sum it
// feeds: every kernel that draws forms the same bits); + 0 turns the -0 of a zero half-width into +0.
template <typename T> MDS_HD void episode_random_offsets(const EpisodeRandom<T>& r, uint32_t g, uint32_t ordinal, T offset[12]) {
  for (uint32_t b = 0; b < 3; ++b) {
    const uint32_t counter[4] = {g, ordinal, b, r.generation};
    uint32_t word[4];
    philox4x32_10(counter, r.key, word);
    for (int k = 0; k < 4; ++k) offset[4 * b + k] = m_mul_rn(episode_random_unit<T>(word[k]), r.half[4 * b + k]) + T(0);
  }
}

template <typename S, typename T> MDS_HD T episode_random_stored(T v) { return (T)(S)v; }

// s: in, the reset image's state of the drone (as load_state reads it); out, its drawn start.  rpy0: the drone's three initial Euler
// angles, read only where an attitude half-width is not 0.
template <typename S, typename T>
MDS_HD void episode_random_start(const EpisodeRandom<T>& r, uint32_t g, uint32_t ordinal, const double* rpy0, State<T>& s) {
  T o[12];
  episode_random_offsets(r, g, ordinal, o);
  s.p = {episode_random_stored<S>(s.p.x + o[0]), episode_random_stored<S>(s.p.y + o[1]), episode_random_stored<S>(s.p.z + o[2])};
  if (r.half[3] != T(0) || r.half[4] != T(0) || r.half[5] != T(0)) {          // (the same in every lane: a scalar branch on the device)
    T q[4];
    quat_from_euler<T>((T)rpy0[0] + o[3], (T)rpy0[1] + o[4], (T)rpy0[2] + o[5], q);
    for (int k = 0; k < 4; ++k) s.q[k] = episode_random_stored<S>(q[k]);
  }
  s.v = {episode_random_stored<S>(o[6]), episode_random_stored<S>(o[7]), episode_random_stored<S>(o[8])};
  s.w = {episode_random_stored<S>(o[9]), episode_random_stored<S>(o[10]), episode_random_stored<S>(o[11])};
}

}  // namespace mds
