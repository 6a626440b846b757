// TEST TOOLING ONLY.  dslpid_control<float> / <double> of multidronesim_amd/csrc/mds_math.hpp compiled with g++ (the flags of
// tests/emul/emul.py), driven the way k_dslpid drives it with an observation array: K calls on n drones with the carried DslPidState.
// Never loaded by the multidronesim_amd package; the product path is the HIP library only.
#include "../../multidronesim_amd/csrc/mds_consts.hpp"

using namespace mds;

// gains: P_FOR3 | I_FOR3 | D_FOR3 | P_TOR3 | I_TOR3 | D_TOR3 (converted like mds_set_dslpid_gains).  obs [K][n][20], tpos [K][n][3],
// trpy [n][3], rpm [K][n][4].  mem [n][9] = last_rpy3 | integral_pos_e3 | integral_rpy_e3 per drone, in T-representable doubles: read
// before the first call and written back after the last, so a run can be continued.
template <typename T>
static void dslpid_run(const mds_config* cfg, const mds_geometric_gains* gg, const double* gains, int n, int K, const double* obs,
                       const double* tpos, const double* trpy, double* mem, double* rpm) {
  Consts<T> c;
  fill_consts(*cfg, *gg, c);
  DslPidGains<T> g;
  for (int k = 0; k < 3; ++k) {
    g.Pf[k] = (T)gains[k]; g.If[k] = (T)gains[3 + k]; g.Df[k] = (T)gains[6 + k];
    g.Pt[k] = (T)gains[9 + k]; g.It[k] = (T)gains[12 + k]; g.Dt[k] = (T)gains[15 + k];
  }
  const T ctrl_dt = (T)(1.0 / cfg->ctrl_freq);      // launch_dslpid
  for (int i = 0; i < n; ++i) {
    double* m = mem + 9 * i;
    DslPidState<T> P;
    P.last_rpy = {(T)m[0], (T)m[1], (T)m[2]};
    P.int_pos = {(T)m[3], (T)m[4], (T)m[5]};
    P.int_rpy = {(T)m[6], (T)m[7], (T)m[8]};
    for (int k = 0; k < K; ++k) {
      const double* ob = obs + ((size_t)k * n + i) * 20;
      const double* tp = tpos + ((size_t)k * n + i) * 3;
      const V3<T> p = {(T)ob[0], (T)ob[1], (T)ob[2]};
      const T q[4] = {(T)ob[3], (T)ob[4], (T)ob[5], (T)ob[6]};
      const V3<T> v = {(T)ob[10], (T)ob[11], (T)ob[12]};
      const V3<T> pos_e = {((T)tp[0] - T(0)) - p.x, ((T)tp[1] - T(0)) - p.y, ((T)tp[2] - T(0)) - p.z};   // k_dslpid with a zero origin
      T act[4];
      dslpid_control<T>(c, g, ctrl_dt, pos_e, q, v, (T)trpy[3 * i + 2], P, act);
      for (int j = 0; j < 4; ++j) rpm[((size_t)k * n + i) * 4 + j] = act[j];
    }
    m[0] = P.last_rpy.x; m[1] = P.last_rpy.y; m[2] = P.last_rpy.z;
    m[3] = P.int_pos.x; m[4] = P.int_pos.y; m[5] = P.int_pos.z;
    m[6] = P.int_rpy.x; m[7] = P.int_rpy.y; m[8] = P.int_rpy.z;
  }
}

extern "C" {
void dslpid_run_f32(const mds_config* cfg, const mds_geometric_gains* gg, const double* gains, int n, int K, const double* obs,
                    const double* tpos, const double* trpy, double* mem, double* rpm) {
  dslpid_run<float>(cfg, gg, gains, n, K, obs, tpos, trpy, mem, rpm);
}
void dslpid_run_f64(const mds_config* cfg, const mds_geometric_gains* gg, const double* gains, int n, int K, const double* obs,
                    const double* tpos, const double* trpy, double* mem, double* rpm) {
  dslpid_run<double>(cfg, gg, gains, n, K, obs, tpos, trpy, mem, rpm);
}
}
