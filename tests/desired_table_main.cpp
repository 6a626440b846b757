// TEST TOOLING ONLY: host build of the two halves of the yaw-free desired state (csrc/mds_math.hpp: lemniscate_desired8 ahead of the cut,
// desired8_p_rel / desired8_pre behind it), of the time of a table row (lemniscate_table_time) and of the rule the desired-state table
// is decided by (lemniscate_desired_periodic).  Compiled by tests/test_desired_table_cpu.py with g++ -ffp-contract=off
// -DMDS_HOST_UNFUSED_FMA: every product is then rounded on its own on both sides, in the explicit-fma halves (m_fma rounds its product
// under that macro) and in the plain-operator expressions of lemniscate_from_sc<float, true> and geometric_control<float, true>, so equal
// bytes mean the same operations on the same operands in the same association.  (Which of them the device contracts is the other
// half of the argument: the halves state it in m_fma, and the GPU tests compare the rows with the table on and off.)
// Built as a shared library for the comparisons from NumPy, and as a program of its own (this main) that makes the same checks on
// inputs of its own -- the build that also runs under -fsanitize=address,undefined.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../multidronesim_amd/csrc/mds_consts.hpp"

using namespace mds;

constexpr int kOut = 10;       // p_rel.x, p_rel.y, des.v.x, des.v.y, tw.x, tw.y, and the controller's u [4]

// the constants of tests/emul/yaw_free_emul.cpp (CF2P, 100 Hz), the gains apart in x, y and z
static Consts<float> test_consts() {
  mds_config cfg;
  mds_geometric_gains g;
  memset(&cfg, 0, sizeof(cfg));
  cfg.num_envs = 1; cfg.num_drones = 1; cfg.dtype = MDS_F32; cfg.drone_model = MDS_CF2P;
  cfg.pyb_freq = 100; cfg.ctrl_freq = 100;
  cfg.M = 0.027; cfg.L = 0.0397; cfg.KF = 3.16e-10; cfg.KM = 7.94e-12;
  cfg.J[0] = 2.3951e-5; cfg.J[1] = 2.3951e-5; cfg.J[2] = 3.2347e-5;
  cfg.G = 9.8; cfg.thrust2weight = 2.25;
  const double kp[3] = {2.25, 1.75, 2.5}, kv[3] = {3.5, 3.0, 3.25};
  for (int k = 0; k < 3; ++k) { g.Kp[k] = kp[k]; g.Kv[k] = kv[k]; g.KR[k] = 125.0; g.Kw[k] = 10.0; }
  g.g = 9.81; g.max_tilt_angle = 40.0 * M_PI / 180.0;
  Consts<float> c;
  fill_consts(cfg, g, c);
  return c;
}

// in [14]: a, omega, s, c, p [3], q [4] (unit), v [3] (float); the body rate is 0.3 v.  whole: lemniscate_from_sc<float, true>, then p - des.p,
// the tw of geometric_control<float, true> as that function writes it, and the controller on that desired state.  split: through the
// eight values and GeoPre.
constexpr int kIn = 14;
static void one(const Consts<float>& k, const float* in, float* whole, float* split, float* eight) {
  LemniscateParams<float> P = {};
  P.a = in[0];
  P.omega = in[1];
  const float s = in[2], c = in[3];
  const V3<float> p = {in[4], in[5], in[6]}, v = {in[11], in[12], in[13]}, w = {0.3f * in[11], 0.3f * in[12], 0.3f * in[13]};
  const M3<float> R = quat_to_rot(in + 7);
  const Desired<float> des = lemniscate_from_sc<float, true>(P, s, c, 0.0);
  const V3<float> p_rel = p - des.p;
  float uw[4], us[4];
  geometric_control<float, true>(k, p_rel, R, v, w, des, uw, nullptr);
  const float wh[kOut] = {p_rel.x, p_rel.y, des.v.x, des.v.y, des.a.x - k.kp[0] * p_rel.x, des.a.y - k.kp[1] * p_rel.y, uw[0], uw[1], uw[2], uw[3]};
  const LemDesired8<float> d = lemniscate_desired8(P, s, c);
  const V3<float> q_rel = desired8_p_rel(d, p);
  GeoPre<float> pre;
  desired8_pre(d, k.kp[0], k.kp[1], q_rel, R, pre);
  const Desired<float> none = {};
  geometric_control<float, true, true>(k, q_rel, R, v, w, none, us, nullptr, &pre);
  const float h[kOut] = {q_rel.x, q_rel.y, d.vx, d.vy, pre.tw_x, pre.tw_y, us[0], us[1], us[2], us[3]};
  memcpy(whole, wh, sizeof(wh));
  memcpy(split, h, sizeof(h));
  if (eight) memcpy(eight, &d, sizeof(d));
}

extern "C" {
void dt_both(int n, const float* in, float* whole, float* split, float* eight) {
  static_assert(sizeof(LemDesired8<float>) == 32, "eight values, two 16-byte groups");
  const Consts<float> k = test_consts();
  for (int i = 0; i < n; ++i) one(k, in + kIn * i, whole + kOut * i, split + kOut * i, eight + 8 * i);
}
void dt_times(double t0, double dt, int n, double* out) {
  for (int k = 0; k < n; ++k) out[k] = lemniscate_table_time(t0, dt, k);
}
int dt_phase_periodic(const double* params, long n) { return lemniscate_phase_periodic(params, n) ? 1 : 0; }
int dt_desired_periodic(const double* params, long n) { return lemniscate_desired_periodic(params, n) ? 1 : 0; }
}

// ---- the program ----
static unsigned long long g_rng = 0x9e3779b97f4a7c15ull;
static double uni(double lo, double hi) {          // xorshift64*: the inputs need no quality, only spread
  g_rng ^= g_rng >> 12; g_rng ^= g_rng << 25; g_rng ^= g_rng >> 27;
  return lo + (hi - lo) * (double)((g_rng * 0x2545f4914f6cdd1dull) >> 11) / 9007199254740992.0;
}

static long split_mismatches(int n) {
  const Consts<float> k = test_consts();
  long bad = 0;
  for (int i = 0; i < n; ++i) {
    const double th = uni(-3.2, 3.2);
    double q[4], qn = 0.0;
    for (int j = 0; j < 4; ++j) { q[j] = uni(-1.0, 1.0) * (j < 3 ? 0.5 : 1.0); qn += q[j] * q[j]; }
    float in[kIn] = {(float)uni(0.2, 3.0), (float)uni(-3.0, 3.0), (float)sin(th), (float)cos(th),
                     (float)uni(-3.0, 3.0), (float)uni(-3.0, 3.0), (float)uni(0.0, 2.0)};
    for (int j = 0; j < 4; ++j) in[7 + j] = (float)(q[j] / sqrt(qn));
    for (int j = 0; j < 3; ++j) in[11 + j] = (float)uni(-2.0, 2.0);
    float w[kOut], h[kOut];
    one(k, in, w, h, nullptr);
    bad += memcmp(w, h, sizeof(w)) != 0;
  }
  return bad;
}

static long time_mismatches() {
  long bad = 0;
  for (double t0 : {0.0, 0.37, 1234.5}) {
    const double dt = 1.0 / 48.0 + 1e-3;      // (not a power of two: the sums round)
    std::vector<double> got(300);             // exactly 300: a write past them is the sanitizer's to report
    dt_times(t0, dt, (int)got.size(), got.data());
    double t = t0;
    for (size_t k = 0; k < got.size(); ++k, t = t + dt) bad += memcmp(&t, &got[k], sizeof(double)) != 0;
  }
  return bad;
}

// the rule restated: brute force over every pair of rows 64 apart
static bool periodic_ref(const std::vector<double>& P, long n, bool with_a) {
  bool ok = true;
  for (long i = 0; i + 64 < n; ++i)
    ok = ok && P[7 * i + 1] == P[7 * (i + 64) + 1] && P[7 * i + 6] == P[7 * (i + 64) + 6] && (!with_a || P[7 * i] == P[7 * (i + 64)]);
  return ok;
}
static long rule_mismatches() {
  long bad = 0;
  const long sizes[] = {1, 63, 64, 65, 100, 128, 259};
  for (long n : sizes) {
    std::vector<double> P((size_t)7 * n);                  // exactly n rows
    for (long i = 0; i < n; ++i) {
      for (int k = 0; k < 7; ++k) P[7 * i + k] = uni(-2, 2);              // the centres and the yaw rate are free
      P[7 * i] = 1.0 + 0.01 * (double)(i % 64);
      P[7 * i + 1] = 0.5 + 0.01 * (double)(i % 64);
      P[7 * i + 6] = 0.1 * (double)(i % 64) - 3.0;
    }
    bad += !lemniscate_desired_periodic(P.data(), n) || !lemniscate_phase_periodic(P.data(), n);
    for (int col : {0, 1, 6})
      for (long row : {64L, n - 1}) {
        if (row < 0 || row >= n) continue;
        std::vector<double> Q = P;
        Q[7 * row + col] += 1e-9;
        bad += lemniscate_phase_periodic(Q.data(), n) != periodic_ref(Q, n, false);
        bad += lemniscate_desired_periodic(Q.data(), n) != periodic_ref(Q, n, true);
        if (n <= 64) bad += !lemniscate_desired_periodic(Q.data(), n);              // (no partner 64 away: nothing to decide)
        else if (col == 0) bad += lemniscate_desired_periodic(Q.data(), n) || !lemniscate_phase_periodic(Q.data(), n);
        else bad += lemniscate_desired_periodic(Q.data(), n) || lemniscate_phase_periodic(Q.data(), n);
      }
  }
  return bad;
}

int main() {
  const long bad = split_mismatches(100000), badt = time_mismatches(), badr = rule_mismatches();
  printf("%ld unequal outputs, %ld wrong row times, %ld wrong periodicity decisions\n", bad, badt, badr);
  return bad || badt || badr ? 1 : 0;
}
