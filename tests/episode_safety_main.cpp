// Stand-alone driver of the collision causes of the episode rule header (multidronesim_amd/csrc/mds_episode.hpp: episode_barrier,
// fill_episode_safety, episode_safety_test, and the cause word they extend) for tests/test_episode_safety_cpu.py: built with g++
// (-fsanitize=address,undefined), run as a subprocess.  No HIP anywhere.
//
//   episode_safety_main <in> <out> f64|f32
// <in>, float64 little endian: M (env-steps), D, max_steps, safety_radius, zscale, n_obs; then 16 obstacle rows of 4 (centre xyz, radius;
//   the first n_obs count); then M * D drone rows of 16 (state 13 = pos3 | quat4 xyzw | vel3 | body rates3, home 3; world frame, origin 0);
//   then M episode lengths (the length the episode has reached with this step).
// <out>, float64: M flags, M * D cause words, M * D smallest h per drone (+inf with nothing to test).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../multidronesim_amd/csrc/mds_episode.hpp"

static const size_t kHead = 6, kObs = 4 * mds::kEpMaxObstacles, kRow = 16;

template <typename T> static void run(const std::vector<double>& in, std::vector<double>& out) {
  const size_t M = (size_t)in[0], D = (size_t)in[1];
  mds::EpisodeRule<T> rule;
  const double inf = (double)INFINITY;
  mds::fill_episode_rule<T>((int)in[2], -inf, inf, inf, inf, inf, inf, 2.0, 0.0, rule);
  mds::EpisodeSafety<T> set;
  mds::fill_episode_safety<T>(in[3], in[4], (int)in[5], in.data() + kHead, set);
  const double* rows = in.data() + kHead + kObs;
  const double* lengths = rows + M * D * kRow;
  out.assign(M + 2 * M * D, 0.0);
  std::vector<mds::V3<T>> p(D);
  for (size_t m = 0; m < M; ++m) {
    int causes = 0;
    for (size_t d = 0; d < D; ++d) {
      const double* r = rows + (m * D + d) * kRow;
      p[d] = {(T)r[0], (T)r[1], (T)r[2]};
    }
    for (size_t d = 0; d < D; ++d) {
      const double* r = rows + (m * D + d) * kRow;
      mds::State<T> s;
      s.p = p[d];
      for (int k = 0; k < 4; ++k) s.q[k] = (T)r[3 + k];
      s.v = {(T)r[7], (T)r[8], (T)r[9]};
      s.w = {(T)r[10], (T)r[11], (T)r[12]};
      const mds::V3<T> home = {(T)r[13], (T)r[14], (T)r[15]};
      int c = mds::episode_causes(rule, s, s.p.z, home);
      T h_min = (T)INFINITY;
      for (size_t j = 0; j < D; ++j) {                       // the kernel's lane: env-mates, then obstacles (origin 0)
        if (j == d) continue;
        mds::episode_safety_test(mds::episode_barrier<T>(p[j].x - p[d].x, p[j].y - p[d].y, p[j].z - p[d].z, set.inv_zscale, set.neg_ds4_pair),
                                 mds::kEpCausePair, c, h_min);
      }
      for (int k = 0; k < set.n_obs; ++k)
        mds::episode_safety_test(mds::episode_barrier<T>(p[d].x - set.obs[k][0], p[d].y - set.obs[k][1], p[d].z - set.obs[k][2], set.inv_zscale,
                                                         set.obs[k][3]),
                                 mds::kEpCauseObstacle, c, h_min);
      out[M + m * D + d] = c;
      out[M + M * D + m * D + d] = (double)h_min;
      causes |= c;
    }
    out[m] = mds::episode_flags(rule, causes, (int)lengths[m]);
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
  if (in.size() < kHead + kObs || in[5] < 0 || in[5] > mds::kEpMaxObstacles) return 5;
  if (in.size() != kHead + kObs + (size_t)in[0] * (size_t)in[1] * kRow + (size_t)in[0]) return 5;
  if (!strcmp(argv[3], "f64")) run<double>(in, out);
  else if (!strcmp(argv[3], "f32")) run<float>(in, out);
  else return 2;
  FILE* g = fopen(argv[2], "wb");
  if (!g) return 3;
  if (fwrite(out.data(), sizeof(double), out.size(), g) != out.size()) return 4;
  fclose(g);
  return 0;
}
