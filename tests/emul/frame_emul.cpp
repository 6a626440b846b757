// TEST TOOLING ONLY: host build of the rotation-frame functions of csrc/mds_math.hpp (make_frame, rpy_from_rot, thrust_dir and the
// quaternion-only entry points that must agree with them to the bit).  Compiled by tests/test_frame_rpy_cpu.py with g++.
#include "../../multidronesim_amd/csrc/mds_math.hpp"

using namespace mds;

// q [n,4] xyzw, w [n,3] body rates -> out [n,18]:
//   0..2  rpy from the frame        3..5  euler_from_quat(q)
//   6..8  the frame's av            9..11 quat_rotate(q, w)
//  12..14 thrust_dir(frame)        15..17 thrust_dir(q)
template <typename T> static void frame_all(int n, const double* q, const double* w, double* out) {
  for (int i = 0; i < n; ++i) {
    const T qq[4] = {(T)q[4 * i], (T)q[4 * i + 1], (T)q[4 * i + 2], (T)q[4 * i + 3]};
    const V3<T> ww = {(T)w[3 * i], (T)w[3 * i + 1], (T)w[3 * i + 2]};
    const Frame<T> F = make_frame(qq, ww);
    const V3<T> a = rpy_from_rot(F.R, qq), b = euler_from_quat(qq), c = quat_rotate(qq, ww), d = thrust_dir(F), e = thrust_dir(qq);
    const T v[18] = {a.x, a.y, a.z, b.x, b.y, b.z, F.av.x, F.av.y, F.av.z, c.x, c.y, c.z, d.x, d.y, d.z, e.x, e.y, e.z};
    for (int k = 0; k < 18; ++k) out[18 * i + k] = (double)v[k];
  }
}

extern "C" {
void frame_all_f32(int n, const double* q, const double* w, double* out) { frame_all<float>(n, q, w, out); }
void frame_all_f64(int n, const double* q, const double* w, double* out) { frame_all<double>(n, q, w, out); }
}
