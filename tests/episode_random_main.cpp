// Stand-alone driver of the randomised-start header (multidronesim_amd/csrc/mds_episode_random.hpp) for
// tests/test_episode_random_cpu.py: built with g++ (-fsanitize=address,undefined), run as a subprocess.  No HIP anywhere.
//
//   episode_random_main kat
// prints Philox4x32-10 of the three known-answer inputs, one line of four hex words each.
//
//   episode_random_main draw <in> <out> f64|f32
// <in>, float64 little endian: N, seed low word, seed high word, the 12 half-widths; then N rows of 9: g, ordinal, generation (integers
//   below 2^32), the nominal xyz and rpy of the drone.
// <out>, float64: N rows of 25: the 12 s values, then the drawn start 13 = pos3 | quat4 xyzw | vel3 | body rates3 (storage type = T; the
//   image the draw starts from is what the library's reset writes: the position and quat_from_euler<double>(rpy) rounded to T, zero rates).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../multidronesim_amd/csrc/mds_episode_random.hpp"

static int known_answers() {
  const uint32_t in[3][6] = {{0u, 0u, 0u, 0u, 0u, 0u},
                             {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu},
                             {0x243f6a88u, 0x85a308d3u, 0x13198a2e, 0x03707344u, 0xa4093822u, 0x299f31d0u}};
  for (const auto& v : in) {
    uint32_t out[4];
    mds::philox4x32_10(v, v + 4, out);
    printf("%08x %08x %08x %08x\n", out[0], out[1], out[2], out[3]);
  }
  return 0;
}

template <typename T> static void run(const std::vector<double>& in, std::vector<double>& out) {
  const size_t N = (size_t)in[0];
  mds::EpisodeRandom<T> set;
  const uint64_t seed = (uint64_t)in[1] | ((uint64_t)in[2] << 32);
  mds::fill_episode_random<T>(seed, 0u, 0u, &in[3], &in[6], &in[9], &in[12], set);
  out.assign(N * 25, 0.0);
  for (size_t m = 0; m < N; ++m) {
    const double* r = in.data() + 15 + m * 9;
    const uint32_t g = (uint32_t)r[0], ordinal = (uint32_t)r[1];
    set.generation = (uint32_t)r[2];
    double* o = out.data() + m * 25;
    for (uint32_t b = 0; b < 3; ++b) {
      const uint32_t counter[4] = {g, ordinal, b, set.generation};
      uint32_t word[4];
      mds::philox4x32_10(counter, set.key, word);
      for (int k = 0; k < 4; ++k) o[4 * b + k] = (double)mds::episode_random_unit<T>(word[k]);
    }
    double q[4];
    mds::quat_from_euler<double>(r[6], r[7], r[8], q);
    mds::State<T> s;
    s.p = {(T)r[3], (T)r[4], (T)r[5]};
    for (int k = 0; k < 4; ++k) s.q[k] = (T)q[k];
    s.v = {T(0), T(0), T(0)};
    s.w = {T(0), T(0), T(0)};
    mds::episode_random_start<T, T>(set, g, ordinal, r + 6, s);
    const T st[13] = {s.p.x, s.p.y, s.p.z, s.q[0], s.q[1], s.q[2], s.q[3], s.v.x, s.v.y, s.v.z, s.w.x, s.w.y, s.w.z};
    for (int k = 0; k < 13; ++k) o[12 + k] = (double)st[k];
  }
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "kat")) return known_answers();
  if (argc != 5 || strcmp(argv[1], "draw")) return 2;
  FILE* f = fopen(argv[2], "rb");
  if (!f) return 3;
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<double> in((size_t)bytes / sizeof(double)), out;
  if (fread(in.data(), sizeof(double), in.size(), f) != in.size()) return 4;
  fclose(f);
  if (in.size() < 15 || in.size() != 15 + (size_t)in[0] * 9) return 5;
  if (!strcmp(argv[4], "f64")) run<double>(in, out);
  else if (!strcmp(argv[4], "f32")) run<float>(in, out);
  else return 2;
  FILE* g = fopen(argv[3], "wb");
  if (!g) return 3;
  if (fwrite(out.data(), sizeof(double), out.size(), g) != out.size()) return 4;
  fclose(g);
  return 0;
}
