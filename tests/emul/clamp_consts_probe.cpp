// TEST TOOLING ONLY: the host build of csrc/mds_consts.hpp's fill_consts and csrc/mds_math.hpp's m_clamp, for
// tests/test_clamp_consts_cpu.py (compiled there with g++; never loaded by the package).
#include <string.h>

#include "../../multidronesim_amd/csrc/mds_consts.hpp"

using namespace mds;

static void config(int model, mds_config* cfg, mds_geometric_gains* g) {
  memset(cfg, 0, sizeof(*cfg));
  memset(g, 0, sizeof(*g));
  cfg->num_envs = 1; cfg->num_drones = 1; cfg->dtype = MDS_F32; cfg->drone_model = model;
  cfg->pyb_freq = 100; cfg->ctrl_freq = 100;
  cfg->M = 0.027; cfg->L = 0.0397; cfg->KF = 3.16e-10; cfg->KM = 7.94e-12;
  cfg->J[0] = 1.4e-5; cfg->J[1] = 1.4e-5; cfg->J[2] = 2.17e-5;
  cfg->G = 9.8; cfg->thrust2weight = 2.25;
  g->Kp[0] = g->Kp[1] = g->Kp[2] = 2.25;
  g->Kv[0] = g->Kv[1] = g->Kv[2] = 3.5;
  g->KR[0] = 125.0; g->KR[1] = 117.3; g->KR[2] = 0.1;       // (uneven: every half is its own value)
  g->Kw[0] = g->Kw[1] = g->Kw[2] = 10.0;
  g->g = 9.81; g->max_tilt_angle = 40.0 * M_PI / 180.0;
}

// base: arm, kf, kR[0..2], cf2x; got: the five products as fill_consts stores them; want: the expressions the device formed per step
// before the products moved to the host, evaluated here in T on the same rounded constants
template <typename T> static void fields(int model, T* base, T* got, T* want) {
  mds_config cfg;
  mds_geometric_gains g;
  config(model, &cfg, &g);
  Consts<T> c;
  fill_consts(cfg, g, c);
  base[0] = c.arm; base[1] = c.kf; base[2] = c.kR[0]; base[3] = c.kR[1]; base[4] = c.kR[2]; base[5] = (T)c.cf2x;
  got[0] = c.arm_kf; got[1] = c.arm_sqh_kf; got[2] = c.kR_half[0]; got[3] = c.kR_half[1]; got[4] = c.kR_half[2];
  volatile T arm = c.arm, kf = c.kf, k0 = c.kR[0], k1 = c.kR[1], k2 = c.kR[2];
  want[0] = arm * kf;
  want[1] = arm * T(0.70710678118654752440) * kf;
  want[2] = T(-0.5) * k0;
  want[3] = T(0.5) * k1;
  want[4] = T(-0.5) * k2;
}

extern "C" {
void probe_fields_f32(int model, float* base, float* got, float* want) { fields<float>(model, base, got, want); }
void probe_fields_f64(int model, double* base, double* got, double* want) { fields<double>(model, base, got, want); }
void probe_clamp_f32(const float* x, int n, float lo, float hi, float* out) {
  for (int i = 0; i < n; ++i) out[i] = m_clamp(x[i], lo, hi);
}
void probe_clamp_f64(const double* x, int n, double lo, double hi, double* out) {
  for (int i = 0; i < n; ++i) out[i] = m_clamp(x[i], lo, hi);
}
}
