// Stand-alone driver of the action-noise header (multidronesim_amd/csrc/mds_policy_noise.hpp) for tests/test_episode_sample_cpu.py:
// built with g++ (-fsanitize=address,undefined), run as a subprocess.  No HIP anywhere.  Files are float64, little endian; 32-bit
// words travel as doubles (exact).
//
//   episode_sample_main <in> <out> f64|f32 words
// <in>: n, then n * 4 words.  <out>: n * 4 eps of policy_noise_box_muller.
//
//   episode_sample_main <in> <out> f64|f32 draw
// <in>: n, seed low word, seed high word, first, epoch, rpm_base, rpm_scale, log_std[4]; then n rows of i, ordinal, length, y[4].
// <out>: per row 17 values: the block's 4 words, eps[4], a[4], logp, rpm[4] (g = first + i).
//
//   episode_sample_main <in> <out> f64|f32 stream
// <in>: n, seed low word, seed high word, ordinal, length, epoch.  <out>: n * 4 eps of g = 0 .. n-1.
//
//   episode_sample_main <in> <out> f64|f32 philox
// <in>: n, key[2]; then n counters of 4.  <out>: n * 4 words of philox4x32_10 (the generator the start draws use).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../multidronesim_amd/csrc/mds_policy.hpp"
#include "../multidronesim_amd/csrc/mds_policy_noise.hpp"

static uint32_t word(double v) { return (uint32_t)(uint64_t)v; }

template <typename T> static int run_words(const std::vector<double>& in, std::vector<double>& out) {
  if (in.empty() || in.size() != 1 + 4 * (size_t)in[0]) return 5;
  const size_t n = (size_t)in[0];
  out.resize(n * 4);
  for (size_t i = 0; i < n; ++i) {
    const uint32_t w[4] = {word(in[1 + 4 * i]), word(in[2 + 4 * i]), word(in[3 + 4 * i]), word(in[4 + 4 * i])};
    T eps[4];
    mds::policy_noise_box_muller<T>(w, eps);
    for (int k = 0; k < 4; ++k) out[4 * i + k] = (double)eps[k];
  }
  return 0;
}

template <typename T> static int run_draw(const std::vector<double>& in, std::vector<double>& out) {
  if (in.size() < 11 || in.size() != 11 + 7 * (size_t)in[0]) return 5;
  const size_t n = (size_t)in[0];
  mds::PolicyNoise<T> p;
  mds::fill_policy_noise<T>((uint64_t)word(in[1]) | ((uint64_t)word(in[2]) << 32), word(in[3]), word(in[4]), in.data() + 7, p);
  out.resize(n * 17);
  for (size_t i = 0; i < n; ++i) {
    const double* row = in.data() + 11 + 7 * i;
    const uint32_t g = p.first + word(row[0]);
    const T y[4] = {(T)row[3], (T)row[4], (T)row[5], (T)row[6]};
    uint32_t w[4];
    T eps[4], a[4], rpm[4];
    mds::policy_noise_words(p.key, g, word(row[1]), word(row[2]), p.epoch, w);
    mds::policy_noise_eps(p, g, word(row[1]), word(row[2]), eps);
    const T logp = mds::policy_noise_sample(p, y, eps, a);
    mds::policy_rpm(a, (T)in[5], (T)in[6], rpm);
    double* o = out.data() + 17 * i;
    for (int k = 0; k < 4; ++k) {
      o[k] = (double)w[k];
      o[4 + k] = (double)eps[k];
      o[8 + k] = (double)a[k];
      o[13 + k] = (double)rpm[k];
    }
    o[12] = (double)logp;
  }
  return 0;
}

template <typename T> static int run_stream(const std::vector<double>& in, std::vector<double>& out) {
  if (in.size() != 6) return 5;
  const size_t n = (size_t)in[0];
  const double zero[4] = {0.0, 0.0, 0.0, 0.0};
  mds::PolicyNoise<T> p;
  mds::fill_policy_noise<T>((uint64_t)word(in[1]) | ((uint64_t)word(in[2]) << 32), 0u, word(in[5]), zero, p);
  out.resize(n * 4);
  for (size_t i = 0; i < n; ++i) {
    T eps[4];
    mds::policy_noise_eps(p, (uint32_t)i, word(in[3]), word(in[4]), eps);
    for (int k = 0; k < 4; ++k) out[4 * i + k] = (double)eps[k];
  }
  return 0;
}

static int run_philox(const std::vector<double>& in, std::vector<double>& out) {
  if (in.size() < 3 || in.size() != 3 + 4 * (size_t)in[0]) return 5;
  const size_t n = (size_t)in[0];
  const uint32_t key[2] = {word(in[1]), word(in[2])};
  out.resize(n * 4);
  for (size_t i = 0; i < n; ++i) {
    const uint32_t c[4] = {word(in[3 + 4 * i]), word(in[4 + 4 * i]), word(in[5 + 4 * i]), word(in[6 + 4 * i])};
    uint32_t w[4];
    mds::philox4x32_10(c, key, w);
    for (int k = 0; k < 4; ++k) out[4 * i + k] = (double)w[k];
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 5) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<double> in((size_t)bytes / sizeof(double)), out;
  if (fread(in.data(), sizeof(double), in.size(), f) != in.size()) return 4;
  fclose(f);
  const bool f64 = !strcmp(argv[3], "f64");
  if (!f64 && strcmp(argv[3], "f32")) return 2;
  int rc;
  if (!strcmp(argv[4], "words")) rc = f64 ? run_words<double>(in, out) : run_words<float>(in, out);
  else if (!strcmp(argv[4], "draw")) rc = f64 ? run_draw<double>(in, out) : run_draw<float>(in, out);
  else if (!strcmp(argv[4], "stream")) rc = f64 ? run_stream<double>(in, out) : run_stream<float>(in, out);
  else if (!strcmp(argv[4], "philox")) rc = run_philox(in, out);
  else return 2;
  if (rc) return rc;
  FILE* g = fopen(argv[2], "wb");
  if (!g) return 3;
  if (fwrite(out.data(), sizeof(double), out.size(), g) != out.size()) return 4;
  fclose(g);
  return 0;
}
