// Stand-alone driver of the policy header (multidronesim_amd/csrc/mds_policy.hpp) for tests/test_episode_policy_cpu.py: built with g++
// (-fsanitize=address,undefined), run as a subprocess.  No HIP anywhere.
//
//   episode_policy_main <in> <out> f64|f32 direct|fixed
// direct: policy_eval on the weights as given (any width).  fixed: the weights zero-padded to the instantiated width that holds them
// (policy_pad), put into the device layout (policy_device_layout) and evaluated by policy_eval_w<W> -- what the kernels do.
// <in>, float64 little endian: n (rows), n_hidden, width, activation, rpm_base, rpm_scale; the policy's weights as torch packs them;
//   n observation rows of 20; n world-frame targets of 3.
// <out>, float64: n * 4 network outputs y, n * 4 commanded RPM.
//
//   episode_policy_main <in> <out> f64|f32 tanh
// <in>: n, then n arguments; <out>: n values of m_tanh.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../multidronesim_amd/csrc/mds_policy.hpp"

template <typename T> static int run(const std::vector<double>& in, std::vector<double>& out, bool fixed) {
  if (in.size() < 6) return 5;
  const size_t n = (size_t)in[0];
  const int n_hidden = (int)in[1], width = (int)in[2], activation = (int)in[3];
  if (n_hidden < 1 || n_hidden > 2 || width < 1 || width > mds::kPolicyMaxWidth) return 5;
  const size_t nw = (size_t)mds::policy_n_weights(n_hidden, width);
  if (in.size() != 6 + nw + n * 23) return 5;
  const double* wsrc = in.data() + 6;
  const double* rows = wsrc + nw;
  const double* targets = rows + n * 20;
  const int W = mds::policy_device_width(width);
  std::vector<T> w(nw);
  for (size_t k = 0; k < nw; ++k) w[k] = (T)wsrc[k];
  std::vector<T> padded((size_t)mds::policy_n_weights(n_hidden, W)), dev(padded.size());
  mds::policy_pad(w.data(), n_hidden, width, W, padded.data());
  mds::policy_device_layout(padded.data(), n_hidden, W, dev.data());
  out.assign(n * 8, 0.0);
  for (size_t i = 0; i < n; ++i) {
    T o[20], x[mds::kPolicyIn], y[mds::kPolicyOut], rpm[mds::kPolicyOut];
    for (int k = 0; k < 20; ++k) o[k] = (T)rows[i * 20 + k];
    mds::policy_features_obs(o, mds::V3<T>{(T)targets[3 * i], (T)targets[3 * i + 1], (T)targets[3 * i + 2]}, x);
    if (!fixed) mds::policy_eval<T>((const T*)w.data(), n_hidden, width, activation, x, y);
    else if (W == 32) mds::policy_eval_w<T, 32>((const T*)dev.data(), n_hidden, activation, x, y);
    else mds::policy_eval_w<T, 64>((const T*)dev.data(), n_hidden, activation, x, y);
    mds::policy_rpm(y, (T)in[4], (T)in[5], rpm);
    for (int k = 0; k < 4; ++k) {
      out[i * 4 + k] = (double)y[k];
      out[n * 4 + i * 4 + k] = (double)rpm[k];
    }
  }
  return 0;
}

template <typename T> static int run_tanh(const std::vector<double>& in, std::vector<double>& out) {
  if (in.empty() || in.size() != 1 + (size_t)in[0]) return 5;
  out.resize((size_t)in[0]);
  for (size_t i = 0; i < out.size(); ++i) out[i] = (double)mds::m_tanh((T)in[1 + i]);
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
  if (!strcmp(argv[4], "tanh")) rc = f64 ? run_tanh<double>(in, out) : run_tanh<float>(in, out);
  else if (!strcmp(argv[4], "direct") || !strcmp(argv[4], "fixed"))
    rc = f64 ? run<double>(in, out, argv[4][0] == 'f') : run<float>(in, out, argv[4][0] == 'f');
  else return 2;
  if (rc) return rc;
  FILE* g = fopen(argv[2], "wb");
  if (!g) return 3;
  if (fwrite(out.data(), sizeof(double), out.size(), g) != out.size()) return 4;
  fclose(g);
  return 0;
}
