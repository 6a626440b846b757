// Stand-alone driver of the episode rule header (multidronesim_amd/csrc/mds_episode.hpp) for tests/test_episode_cpu.py: built with g++
// (-fsanitize=address,undefined), run as a subprocess.  No HIP anywhere.
//
//   episode_rule_main <in> <out> f64|f32
// <in>, float64 little endian: M (env-steps), D, max_steps, z_min, z_max, max_dist, max_tilt, max_speed, max_rate, reward_r0, term_penalty;
//   then M * D drone rows of 19 (state 13 = pos3 | quat4 xyzw | vel3 | body rates3, home 3, target 3; world frame, origin 0);
//   then M episode lengths (the length the episode has reached with this step).
// <out>, float64: M flags, M rewards, M * D cause bits.
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

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<double> in((size_t)bytes / sizeof(double)), out;
  if (fread(in.data(), sizeof(double), in.size(), f) != in.size()) return 4;
  fclose(f);
  if (in.size() < 11 || in.size() != 11 + (size_t)in[0] * (size_t)in[1] * 19 + (size_t)in[0]) return 5;
  if (!strcmp(argv[3], "f64")) run<double>(in, out);
  else if (!strcmp(argv[3], "f32")) run<float>(in, out);
  else return 2;
  FILE* g = fopen(argv[2], "wb");
  if (!g) return 3;
  if (fwrite(out.data(), sizeof(double), out.size(), g) != out.size()) return 4;
  fclose(g);
  return 0;
}
