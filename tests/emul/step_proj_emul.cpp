// TEST TOOLING ONLY: host build of the short forms of csrc/mds_math.hpp that the fused step uses -- m_sincos_reduced / m_sincos_small
// beside m_sincos, and reject() / the un-normalised b1d beside the double cross products the reference controller writes
// (control/geometric.py:91-99).  Compiled by tests/test_step_projections_cpu.py with g++.
#include "../../multidronesim_amd/csrc/mds_math.hpp"

using namespace mds;

// (a x b) x a as the reference writes it
template <typename T> static V3<T> reject_by_cross(V3<T> b, V3<T> a) { return cross(cross(a, b), a); }

template <typename T> static V3<T> unit(V3<T> v) { return m_rsqrt(dot(v, v)) * v; }
template <typename T> static V3<double> widen(V3<T> v) { return {(double)v.x, (double)v.y, (double)v.z}; }
static void put(double* o, V3<double> v) { o[0] = v.x; o[1] = v.y; o[2] = v.z; }

extern "C" {

// out [n,6]: m_sincos (s, c), m_sincos_reduced (s, c), m_sincos_small (s, c)
void sincos_three_f32(int n, const float* x, float* out) {
  for (int i = 0; i < n; ++i) {
    m_sincos(x[i], &out[6 * i], &out[6 * i + 1]);
    m_sincos_reduced(x[i], &out[6 * i + 2], &out[6 * i + 3]);
    m_sincos_small(x[i], &out[6 * i + 4], &out[6 * i + 5]);
  }
}

// The desired frame's derivatives as geometric_control forms them, from raw inputs f [n,3] (the force direction, any length),
// yaw [n], fd [n,3] (f_dot), in_ [n,3] (inner): b3d = unit(f), b2d = unit(b3d x b1c) in fp32 as the controller normalises them; then
// on those SAME fp32 unit vectors
//   out [n, 0.. 2] reject(fd, b3d) fp32            [ 3.. 5] (b3d x fd) x b3d fp32            [ 6.. 8] (b3d x fd) x b3d in double
//   out [n, 9..11] reject(in_, b2d) fp32           [12..14] (b2d x in_) x b2d fp32           [15..17] (b2d x in_) x b2d in double
//   out [n,18..20] b2d x b3d fp32                  [21..23] unit(b2d x b3d) fp32             [24..26] unit(b2d x b3d) in double
void frame_derivs(int n, const double* f, const double* yaw, const double* fd, const double* in_, double* out) {
  for (int i = 0; i < n; ++i) {
    const V3<float> fw = {(float)f[3 * i], (float)f[3 * i + 1], (float)f[3 * i + 2]};
    const V3<float> b1c = {cosf((float)yaw[i]), sinf((float)yaw[i]), 0.0f};
    const V3<float> b3d = unit(fw), b2d = unit(cross(b3d, b1c));
    const V3<float> fdot = {(float)fd[3 * i], (float)fd[3 * i + 1], (float)fd[3 * i + 2]};
    const V3<float> inner = {(float)in_[3 * i], (float)in_[3 * i + 1], (float)in_[3 * i + 2]};
    double* o = out + 27 * i;
    put(o + 0, widen(reject(fdot, b3d)));
    put(o + 3, widen(reject_by_cross(fdot, b3d)));
    put(o + 6, reject_by_cross(widen(fdot), widen(b3d)));
    put(o + 9, widen(reject(inner, b2d)));
    put(o + 12, widen(reject_by_cross(inner, b2d)));
    put(o + 15, reject_by_cross(widen(inner), widen(b2d)));
    put(o + 18, widen(cross(b2d, b3d)));
    put(o + 21, widen(unit(cross(b2d, b3d))));
    put(o + 24, unit(cross(widen(b2d), widen(b3d))));
  }
}
}
