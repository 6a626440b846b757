// Stand-alone driver of the episode rule header (multidronesim_amd/csrc/mds_episode.hpp) for tests/test_episode_cpu.py: built with g++
// (-fsanitize=address,undefined), run as a subprocess.  No HIP anywhere.
//
//   episode_rule_main <in> <out> f64|f32
// <in>, float64 little endian: M (env-steps), D, max_steps, z_min, z_max, max_dist, max_tilt, max_speed, max_rate, reward_r0, term_penalty;
//   then M * D drone rows of 19 (state 13 = pos3 | quat4 xyzw | vel3 | body rates3, home 3, target 3; world frame, origin 0);
//   then M episode lengths (the length the episode has reached with this step).
// <out>, float64: M flags, M rewards, M * D cause bits.
//
//   episode_rule_main <in> <out> f64|f32 tally
// the env's step with its counters carried (episode_env_step over an EpisodeTally), K steps of E envs from zeroed counters.
// <in>, float64: K, E, max_steps, term_penalty; then K * E cause words (the OR over the env's drones); then K * E term sums.
// <out>, float64: K * E flags, K * E rewards (step k of env e at k * E + e), then length, count, sum_length, ret, sum_return of every
//   env: 5 * E.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../multidronesim_amd/csrc/mds_episode.hpp"

template <typename T> static void run(const std::vector<double>& in, std::vector<double>& out) {
  const size_t M = (size_t)in[0], D = (size_t)in[1];
  mds::EpisodeRule<T> rule;
  mds::fill_episode_rule<T>((int)in[2], in[3], in[4], in[5], in[6], in[7], in[8], in[9], in[10], rule);
  const double* rows = in.data() + 11;
  const double* lengths = rows + M * D * 19;
  out.assign(2 * M + M * D, 0.0);
  for (size_t m = 0; m < M; ++m) {
    int causes = 0;
    T sum = T(0);
    for (size_t d = 0; d < D; ++d) {
      const double* r = rows + (m * D + d) * 19;
      mds::State<T> s;
      s.p = {(T)r[0], (T)r[1], (T)r[2]};
      for (int k = 0; k < 4; ++k) s.q[k] = (T)r[3 + k];
      s.v = {(T)r[7], (T)r[8], (T)r[9]};
      s.w = {(T)r[10], (T)r[11], (T)r[12]};
      const mds::V3<T> home = {(T)r[13], (T)r[14], (T)r[15]}, target = {(T)r[16], (T)r[17], (T)r[18]};
      const int c = mds::episode_causes(rule, s, s.p.z, home);
      out[2 * M + m * D + d] = c;
      causes |= c;
      sum += mds::episode_reward_term(rule, s.p, target);
    }
    const int flags = mds::episode_flags(rule, causes, (int)lengths[m]);
    out[m] = flags;
    out[M + m] = (double)mds::episode_reward(rule, sum, flags);
  }
}

template <typename T> static int run_tally(const std::vector<double>& in, std::vector<double>& out) {
  const size_t K = (size_t)in[0], E = (size_t)in[1];
  mds::EpisodeRule<T> rule;
  mds::fill_episode_rule<T>((int)in[2], -INFINITY, INFINITY, INFINITY, INFINITY, INFINITY, INFINITY, 2.0, in[3], rule);
  const double* causes = in.data() + 4;
  const double* sums = causes + K * E;
  std::vector<mds::EpisodeTally<T>> tally(E);
  out.assign(2 * K * E + 5 * E, 0.0);
  for (size_t k = 0; k < K; ++k)
    for (size_t e = 0; e < E; ++e) {
      const size_t m = k * E + e;
      const mds::EpisodeStep<T> st = mds::episode_env_step(rule, (int)causes[m], (T)sums[m], tally[e]);
      if (st.done != ((st.flags & (mds::kEpTerminated | mds::kEpTruncated)) != 0)) return 6;
      out[m] = st.flags;
      out[K * E + m] = (double)st.reward;
    }
  double* c = out.data() + 2 * K * E;
  for (size_t e = 0; e < E; ++e) {
    c[e] = tally[e].length; c[E + e] = tally[e].count; c[2 * E + e] = tally[e].sum_length;
    c[3 * E + e] = (double)tally[e].ret; c[4 * E + e] = (double)tally[e].sum_return;
  }
  return 0;
}

int main(int argc, char** argv) {
  const bool tally = argc == 5 && !strcmp(argv[4], "tally");
  if (argc != 4 && !tally) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<double> in((size_t)bytes / sizeof(double)), out;
  if (fread(in.data(), sizeof(double), in.size(), f) != in.size()) return 4;
  fclose(f);
  if (tally) {
    if (in.size() < 4 || in.size() != 4 + 2 * (size_t)in[0] * (size_t)in[1]) return 5;
    const int rc = !strcmp(argv[3], "f64") ? run_tally<double>(in, out) : !strcmp(argv[3], "f32") ? run_tally<float>(in, out) : 2;
    if (rc) return rc;
  } else if (in.size() < 11 || in.size() != 11 + (size_t)in[0] * (size_t)in[1] * 19 + (size_t)in[0]) return 5;
  else if (!strcmp(argv[3], "f64")) run<double>(in, out);
  else if (!strcmp(argv[3], "f32")) run<float>(in, out);
  else return 2;
  FILE* g = fopen(argv[2], "wb");
  if (!g) return 3;
  if (fwrite(out.data(), sizeof(double), out.size(), g) != out.size()) return 4;
  fclose(g);
  return 0;
}
