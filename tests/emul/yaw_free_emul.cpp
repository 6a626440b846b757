// TEST TOOLING ONLY: host build of the yaw-free forms of csrc/mds_math.hpp (lemniscate_local<T, true>, geometric_control<T, true>)
// beside the general forms at yaw_rate = +-0.  Compiled by tests/test_yaw_free_cpu.py with g++: as a shared library for the
// comparisons from NumPy, and with -DYAW_FREE_MAIN as a stand-alone program that makes the same comparison on inputs of its own
// (the build that runs under -fsanitize=address,undefined).
#include <stdio.h>
#include <string.h>

#include "../../multidronesim_amd/csrc/mds_consts.hpp"

using namespace mds;

// the constants of tests/emul/mds_emul.cpp's emul_default_config (CF2P, 100 Hz)
template <typename T> static Consts<T> default_consts() {
  mds_config cfg;
  mds_geometric_gains g;
  memset(&cfg, 0, sizeof(cfg));
  cfg.num_envs = 1; cfg.num_drones = 1; cfg.dtype = MDS_F32; cfg.drone_model = MDS_CF2P;
  cfg.pyb_freq = 100; cfg.ctrl_freq = 100;
  cfg.M = 0.027; cfg.L = 0.0397; cfg.KF = 3.16e-10; cfg.KM = 7.94e-12;
  cfg.J[0] = 2.3951e-5; cfg.J[1] = 2.3951e-5; cfg.J[2] = 3.2347e-5;
  cfg.G = 9.8; cfg.thrust2weight = 2.25;
  cfg.drag_coeff[0] = 9.1785e-7; cfg.drag_coeff[1] = 9.1785e-7; cfg.drag_coeff[2] = 10.311e-7;
  for (int k = 0; k < 3; ++k) { g.Kp[k] = 2.25; g.Kv[k] = 3.5; g.KR[k] = 125.0; g.Kw[k] = 10.0; }
  g.g = 9.81; g.max_tilt_angle = 40.0 * M_PI / 180.0;
  Consts<T> c;
  fill_consts(cfg, g, c);
  return c;
}

constexpr int kGeoOut = 21;   // rpm 4 | u 4 | force | w_des 3 | b1d 3 | b2d 3 | b3d 3

// One controller call: obs [20] (the observation row; obs[13:16] is read as the body rate, as the reference does), des [11] = p, v, a,
// yaw, yaw_rate with v.z = a.z = yaw = 0 and yaw_rate = +-0.  out [21] in T.
template <typename T, bool Y0> static void geo_one(const Consts<T>& c, const double* o, const double* d, T* out) {
  const T q[4] = {(T)o[3], (T)o[4], (T)o[5], (T)o[6]};
  const M3<T> R = quat_to_rot(q);
  Desired<T> D;
  D.p = {(T)d[0], (T)d[1], (T)d[2]};
  D.v = {(T)d[3], (T)d[4], (T)d[5]};
  D.a = {(T)d[6], (T)d[7], (T)d[8]};
  D.yaw = (T)d[9];
  D.yaw_rate = (T)d[10];
  T u[4], act[4];
  GeoAux<T> A;
  geometric_control<T, Y0>(c, V3<T>{(T)o[0], (T)o[1], (T)o[2]} - D.p, R, V3<T>{(T)o[10], (T)o[11], (T)o[12]},
                           V3<T>{(T)o[13], (T)o[14], (T)o[15]}, D, u, &A);
  input_to_action(c, u, act);
  for (int k = 0; k < 4; ++k) { out[k] = act[k]; out[4 + k] = u[k]; }
  out[8] = A.force;
  const V3<T> v[4] = {A.w_des, A.b1d, A.b2d, A.b3d};
  for (int k = 0; k < 4; ++k) { out[9 + 3 * k] = v[k].x; out[10 + 3 * k] = v[k].y; out[11 + 3 * k] = v[k].z; }
}

template <typename T> static void geo_both(int n, const double* obs, const double* des, T* gen, T* y0) {
  const Consts<T> c = default_consts<T>();
  for (int i = 0; i < n; ++i) {
    geo_one<T, false>(c, obs + 20 * i, des + 11 * i, gen + kGeoOut * i);
    geo_one<T, true>(c, obs + 20 * i, des + 11 * i, y0 + kGeoOut * i);
  }
}

// P [n,7] = (a, omega, cx, cy, cz, yaw_rate, phase_shift) as mds_set_lemniscate takes them; out [n,11] in T (local frame: no centre)
template <typename T> static void lem_both(int n, const double* P, const double* t, T* gen, T* y0) {
  for (int i = 0; i < n; ++i) {
    const double* p = P + 7 * i;
    const LemniscateParams<T> L = {(T)p[0], (T)p[1], (T)p[2], (T)p[3], (T)p[4], (T)p[5], (T)p[6]};
    const Desired<T> a = lemniscate_local<T, false>(L, t[i]), b = lemniscate_local<T, true>(L, t[i]);
    const Desired<T>* two[2] = {&a, &b};
    T* outs[2] = {gen + 11 * i, y0 + 11 * i};
    for (int k = 0; k < 2; ++k) {
      const Desired<T>& d = *two[k];
      const T row[11] = {d.p.x, d.p.y, d.p.z, d.v.x, d.v.y, d.v.z, d.a.x, d.a.y, d.a.z, d.yaw, d.yaw_rate};
      memcpy(outs[k], row, sizeof(row));
    }
  }
}

extern "C" {
void yf_geo_f32(int n, const double* obs, const double* des, float* gen, float* y0) { geo_both<float>(n, obs, des, gen, y0); }
void yf_geo_f64(int n, const double* obs, const double* des, double* gen, double* y0) { geo_both<double>(n, obs, des, gen, y0); }
void yf_lem_f32(int n, const double* P, const double* t, float* gen, float* y0) { lem_both<float>(n, P, t, gen, y0); }
void yf_lem_f64(int n, const double* P, const double* t, double* gen, double* y0) { lem_both<double>(n, P, t, gen, y0); }
}

#if defined(YAW_FREE_MAIN)
// The same comparison as a program: inputs from a 64-bit LCG (the distribution of the Python test, roughly), both forms, every
// output compared with ==; prints the counts and returns 1 on a mismatch.
static uint64_t g_seed = 0x9E3779B97F4A7C15ull;
static double uni(double lo, double hi) {
  g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
  return lo + (hi - lo) * (double)(g_seed >> 11) * (1.0 / 9007199254740992.0);
}

template <typename T> static int run(int n, const char* name) {
  int bad = 0, same_bytes = 0;
  const Consts<T> c = default_consts<T>();
  for (int i = 0; i < n; ++i) {
    double o[20] = {0}, d[11] = {0}, P[7], t = uni(0.0, 40.0);
    for (int k = 0; k < 3; ++k) o[k] = uni(-2.0, 2.0);
    double q[4], qn = 0.0;
    for (int k = 0; k < 4; ++k) { q[k] = uni(-1.0, 1.0) * (k < 3 ? 0.5 : 1.0); qn += q[k] * q[k]; }
    for (int k = 0; k < 4; ++k) o[3 + k] = q[k] / sqrt(qn);
    for (int k = 0; k < 3; ++k) { o[10 + k] = uni(-2.0, 2.0); o[13 + k] = uni(-3.0, 3.0); }
    d[0] = uni(-1.0, 1.0); d[1] = uni(-1.0, 1.0); d[3] = uni(-1.5, 1.5); d[4] = uni(-1.5, 1.5); d[6] = uni(-5.0, 5.0); d[7] = uni(-5.0, 5.0);
    d[10] = (i & 1) ? -0.0 : 0.0;
    // the degenerate states of the Python comparison
    if (i % 7 == 0) { memset(o, 0, sizeof(o)); o[6] = 1.0; }            // identity attitude at rest
    if (i % 11 == 0) { o[0] = d[0]; o[1] = d[1]; o[2] = 0.0; }          // p_rel = 0
    if (i % 13 == 0) { d[3 + (i / 13) % 2] = 0.0; d[6] = d[7] = 0.0; }  // des.v along one axis
    if (i % 17 == 0) {                                                  // commanded force through zero: f_w.z changes sign at p_rel.z = g / Kp
      const double dz[5] = {-1e-3, -1e-6, 1e-6, 1e-3, 0.5};
      memset(o, 0, sizeof(o)); o[6] = 1.0; memset(d, 0, sizeof(d));
      o[1] = 0.4; o[2] = 9.81 / 2.25 + dz[(i / 17) % 5];
    }
    if (i % 19 == 0) { o[0] = d[0] + 3.0; o[1] = d[1] - 2.5; }          // tilt limit taken: lateral demand well beyond 40 degrees
    T a[kGeoOut], b[kGeoOut];
    geo_one<T, false>(c, o, d, a);
    geo_one<T, true>(c, o, d, b);
    for (int k = 0; k < kGeoOut; ++k) bad += !(a[k] == b[k]);
    same_bytes += memcmp(a, b, sizeof(a)) == 0;
    P[0] = uni(0.5, 2.0); P[1] = uni(0.2, 2.0); P[2] = P[3] = P[4] = 0.0; P[5] = d[10]; P[6] = uni(-3.2, 3.2);
    T la[11], lb[11];
    lem_both<T>(1, P, &t, la, lb);
    for (int k = 0; k < 11; ++k) bad += !(la[k] == lb[k]);
  }
  printf("%s: %d inputs, %d unequal outputs, %d controller results byte-equal\n", name, n, bad, same_bytes);
  return bad;
}

int main() {
  const int bad = run<float>(20000, "float") + run<double>(20000, "double");
  return bad ? 1 : 0;
}
#endif
