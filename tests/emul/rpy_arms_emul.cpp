// TEST TOOLING ONLY: host build of the short arms of csrc/mds_math.hpp's Euler-angle block beside the general arms they stand in for
// (m_atan2_arm, m_asin_arm, rpy_from_rot_arm with the flag the device takes from a wave-wide test, set by hand here).
// Compiled by tests/test_rpy_short_arms_cpu.py with g++.
#include "../../multidronesim_amd/csrc/mds_math.hpp"

using namespace mds;

// m_atan2 as it was written before it had arms (the zero guard a select on the quotient, the fix-ups in line): the general arm has
// to be this to the bit for every input
static float atan2_one_piece(float y, float x) {
  const float ax = fabsf(x), ay = fabsf(y);
  const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
  const float a = mx > 0.0f ? mn * m_rcp(mx) : 0.0f;
  const float z = a * a;
  float p = 2.4567161705e-03f;
  p = fmaf(p, z, -1.4401325081e-02f);
  p = fmaf(p, z, 3.9781171302e-02f);
  p = fmaf(p, z, -7.2348530072e-02f);
  p = fmaf(p, z, 1.0498944039e-01f);
  p = fmaf(p, z, -1.4161228666e-01f);
  p = fmaf(p, z, 1.9985906696e-01f);
  p = fmaf(p, z, -3.3332597024e-01f);
  p = fmaf(p, z, 9.9999988638e-01f);
  float r = p * a;
  r = ay > ax ? 1.57079632679489661923f - r : r;
  r = x < 0.0f ? 3.14159265358979323846f - r : r;
  return copysignf(r, y);
}

extern "C" {

// out [n,4]: the general arm, the short arm, m_atan2 (which picks by the value's own condition on the host), the one-piece form;
// ok [n]: that condition
void atan2_arms_f32(int n, const float* y, const float* x, float* out, int* ok) {
  for (int i = 0; i < n; ++i) {
    out[4 * i] = m_atan2_arm(y[i], x[i], false);
    out[4 * i + 1] = m_atan2_arm(y[i], x[i], true);
    out[4 * i + 2] = m_atan2(y[i], x[i]);
    out[4 * i + 3] = atan2_one_piece(y[i], x[i]);
    ok[i] = m_atan2_in_octant(y[i], x[i]);
  }
}

// out [n,2]: the general arm, the short arm
void asin_arms_f32(int n, const float* x, float* out) {
  for (int i = 0; i < n; ++i) {
    out[2 * i] = m_asin_arm(x[i], false);
    out[2 * i + 1] = m_asin_arm(x[i], true);
  }
}

// q [n,4] xyzw (float64, rounded to fp32 here) -> out [n,10]: rpy by the general path, by the plain block, by rpy_from_rot, R20;
// plain [n]: rpy_is_plain of the matrix
void rpy_arms_f32(int n, const double* q, float* out, int* plain) {
  for (int i = 0; i < n; ++i) {
    const float qq[4] = {(float)q[4 * i], (float)q[4 * i + 1], (float)q[4 * i + 2], (float)q[4 * i + 3]};
    const M3<float> R = quat_to_rot(qq);
    const V3<float> a = rpy_from_rot_arm(R, qq, false), b = rpy_from_rot_arm(R, qq, true), c = rpy_from_rot(R, qq);
    const float v[10] = {a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z, R.m[6]};
    for (int k = 0; k < 10; ++k) out[10 * i + k] = v[k];
    plain[i] = rpy_is_plain(R);
  }
}
}
