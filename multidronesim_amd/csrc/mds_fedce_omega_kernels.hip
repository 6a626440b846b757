// FedCE system identification and the decentralised LQR on the 9-state thrust / body-rate model
// (control/dlqr/decentralized_lqr_omega.py, simulations/EnvGeometricOmega.py fedCE / fedCE_iteration).  Included by mds_api.hip in
// part 2 only, after mds_fedce_kernels.hip (DESIGN.md "FedCE, thrust / body-rate model").  The arithmetic is mds_fedce_omega.hpp.
//
//   k_fedce_omega_identify : one warm-up or exploration phase (T steps) per launch.  16 lanes per drone, 13 live: lane r keeps row r
//                            of the information matrix V, of W = V^-1 and of theta [13, 9] (float64 in every dtype) in registers for
//                            the whole phase.  theta^T z of the forward prediction is a butterfly sum over the row per column, so
//                            every lane of a row sees the same bits and takes rk45_linear's decisions together; rows of different
//                            drones may take different numbers of steps.  The physics and the PID are replicated, lane 0 stores.
//   k_dlqr_omega_rollout   : one CE phase / do_control run per launch, one drone per lane, whole envs per workgroup, error states
//                            through LDS, the ThrustOmega PID memory in registers across the launch.
//   k_dlqr_omega_compute   : DecentralizedLQROmega.compute(obs, skip_low_level) for every env, one call.
//   k_cbf_nominal_dlqr_omega : the same compute(obs, skip_low_level=True) as the nominal controller of the CBF-filtered step
//                            (simulations/CBFTest.py:303-343 with 'dlqr'), from the state planes, into the filter's scratch.
#include <hip/hip_runtime.h>

#include "mds_fedce_omega.hpp"
#include "mds_traj.hpp"

namespace mds {

constexpr int kOmegaM = 9, kOmegaN = 4, kOmegaR = kOmegaM + kOmegaN;

// v[r] for a lane-dependent r without indexing a register array (that would live in scratch); 0 past the end
template <int LEN> __device__ __forceinline__ double lane_pick(const double* v, int r) {
  double out = 0.0;
#pragma unroll
  for (int k = 0; k < LEN; ++k) out = r == k ? v[k] : out;
  return out;
}

struct RowSum16 {
  __device__ __forceinline__ double operator()(double v) const { return row_sum16(v); }
};

// f(e) = theta^T [e; u] with row r of theta on lane r of the 16-lane row: one butterfly sum per column
template <int M, int N> struct RowRhs {
  const double* th_row;
  const double* u;
  int r;
  __device__ __forceinline__ void operator()(const double y[M], double dy[M]) const {
    const double z = r < M ? lane_pick<M>(y, r) : lane_pick<N>(u, r - M);
#pragma unroll
    for (int c = 0; c < M; ++c) dy[c] = row_sum16(th_row[c] * z);
  }
};

struct OmegaDes {
  double yaw;
  V3<double> v, p;
};

// DecentralizedLQROmega.error_state(obs_to_lin_model(obs, 9), x_des) in float64 from the state in the env's dtype
template <typename T> __device__ __forceinline__ void omega_error(const State<T>& s, V3<T> org, const OmegaDes& xd, double e[kOmegaM]) {
  const V3<T> rpy = euler_from_quat(s.q);
  const V3<double> p = {(double)(s.p.x + org.x), (double)(s.p.y + org.y), (double)(s.p.z + org.z)};
  error_state9<double>(V3<double>{(double)rpy.x, (double)rpy.y, (double)rpy.z}, V3<double>{(double)s.v.x, (double)s.v.y, (double)s.v.z},
                       p - xd.p, xd.v, xd.yaw, e);
}

// One warm-up or exploration phase of fedCE_iteration (EnvGeometricOmega.py:143-193, :226-262) for every drone, n_steps steps, wind from
// Consts.  Per step: e_t, the raw u through compute_low_level (body rate = the state's; the PID memory from / to ll), phi = [e_t,
// max(u0, 0) - M G, u1..3] (computeControlFromInput clips u[0] in place, :93), the step, e_{t+1} and -- update 1: every step; 2: every
// step but the launch's first -- rls2_update.  A drone whose forward prediction fails keeps its theta / V / W for that step and gets the
// failure bits or-ed into status[i].  u [T,n,4] float64; xdes [n,9] float64 (NULL: zeros); obs_log [T,n,20] S, theta_log [T,n,13,9]
// float64 and status [n] may be NULL.  COV: the update is theta_update, the covariance form (simulations/CBFTest.py:192, :260), rls_cov_update_row.
template <typename T, typename S, bool DRAG, bool COV = false>
__global__ __launch_bounds__(kFedceBlock) void k_fedce_omega_identify(const Consts<T> c, const double mg, const double ctrl_dt, const int n,
                                                                      const size_t ld, const int n_steps, S* __restrict__ state,
                                                                      const T* __restrict__ origin, T* __restrict__ last_rpm,
                                                                      T* __restrict__ ll, const double* __restrict__ u_in,
                                                                      const double* __restrict__ xdes, const int update,
                                                                      double* __restrict__ Vg, double* __restrict__ Wg,
                                                                      double* __restrict__ thg, S* __restrict__ obs_log,
                                                                      double* __restrict__ theta_log, int32_t* __restrict__ status) {
  constexpr int M = kOmegaM, N = kOmegaN, R = kOmegaR;
  const int gid = blockIdx.x * kFedceBlock + threadIdx.x;
  const int i = gid >> 4, r = gid & 15;
  if (i >= n) return;                        // whole 16-lane rows leave together
  const bool live = r < R;
  State<T> s;
  load_state<S, T>(state, ld, i, s);
  const V3<T> org = load_origin(origin, ld, i);
  T prev[4] = {T(0), T(0), T(0), T(0)}, clipped[4] = {T(0), T(0), T(0), T(0)};
  load_prev_rpm<DRAG>(last_rpm, ld, i, prev);
  LowLevelState<T> L = load_lowlevel(ll, ld, i);
  OmegaDes xd = {0.0, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
  if (xdes) {
    const double* x = xdes + (size_t)i * M;
    xd = {x[2], {x[3], x[4], x[5]}, {x[6], x[7], x[8]}};
  }
  double Vrow[R], Wrow[R], th[M];
  for (int k = 0; k < R; ++k) {
    Vrow[k] = live ? Vg[((size_t)i * R + r) * R + k] : 0.0;
    Wrow[k] = live ? Wg[((size_t)i * R + r) * R + k] : 0.0;
  }
  for (int k = 0; k < M; ++k) th[k] = live ? thg[((size_t)i * R + r) * M + k] : 0.0;
  int bits = 0;
  double e[M];
  omega_error<T>(s, org, xd, e);
  for (int t = 0; t < n_steps; ++t) {
    double phi[R];
    const double* ut = u_in + ((size_t)t * n + i) * 4;
    T uT[4], act[4];
    for (int k = 0; k < 4; ++k) uT[k] = (T)ut[k];
    thrust_omega_control(c, (T)ctrl_dt, uT, s.w, L, act);
    for (int k = 0; k < M; ++k) phi[k] = e[k];
    phi[M] = fmax(ut[0], 0.0) - mg;
    phi[M + 1] = ut[1]; phi[M + 2] = ut[2]; phi[M + 3] = ut[3];
    aviary_step<T, false, DRAG>(c, s, act, prev, clipped);
    double e1[M];
    omega_error<T>(s, org, xd, e1);
    if (update == 1 || (update == 2 && t > 0)) {
      double pred[M];
      int steps, nfev;
      const RowRhs<M, N> f = {th, phi + M, r};
      const int st = rk45_linear<double, M>(f, e1, ctrl_dt, 1e-3, 1e-6, pred, &steps, &nfev);     // from x_tp1 (sic, :119)
      if (st == 0) {
        double innov[M];
        for (int k = 0; k < M; ++k) innov[k] = e1[k] - pred[k];
        if (COV) rls_cov_update_row<M, N>(RowSum16{}, lane_pick<R>(phi, r), phi, innov, th, Vrow, Wrow);
        else rls2_update_row<M, N>(RowSum16{}, lane_pick<R>(phi, r), phi, innov, th, Vrow, Wrow);
      } else {
        bits |= st;
      }
    }
    if (theta_log && live) {
      double* o = theta_log + (((size_t)t * n + i) * R + r) * M;
      for (int k = 0; k < M; ++k) o[k] = th[k];
    }
    if (obs_log && r == 0) {
      T o[kObsDim];
      pack_obs(s, org, clipped, o);
      for (int k = 0; k < 5; ++k) store4<S, T>(obs_log + ((size_t)t * n + i) * kObsDim + 4 * k, o + 4 * k);
    }
    for (int k = 0; k < M; ++k) e[k] = e1[k];
  }
  if (live) {
    for (int k = 0; k < R; ++k) {
      Vg[((size_t)i * R + r) * R + k] = Vrow[k];
      Wg[((size_t)i * R + r) * R + k] = Wrow[k];
    }
    for (int k = 0; k < M; ++k) thg[((size_t)i * R + r) * M + k] = th[k];
  }
  if (r == 0) {
    store_state<S, T>(state, ld, i, s);
    store_lowlevel(ll, ld, i, L);
    if (status && bits) status[i] |= bits;
    if (last_rpm && n_steps > 0) store_last_rpm<DRAG>(last_rpm, ld, i, DRAG ? prev : clipped);
  }
}

// Element of K_e[4j + q][M k + col] in the device layout [E][4][M D][D] (dlqr_kidx with M columns per drone)
template <int M> __host__ __device__ __forceinline__ size_t dlqr_kidx_m(size_t env, int D, int j, int q, int col) {
  return ((env * 4 + (size_t)q) * (size_t)(M * D) + (size_t)col) * (size_t)D + (size_t)j;
}

// u_j = -sum_k K_e[4j:4j+4, 9k:9k+9] e_k (DecentralizedLQROmega.compute, :220-223: per-drone products, summed over the drones in order)
template <typename T, int M>
__device__ __forceinline__ void dlqr_input_m(const T* __restrict__ K, size_t env, int D, int j, const T (*se)[M], T u[4]) {
  for (int q = 0; q < 4; ++q) u[q] = T(0);
  for (int k = 0; k < D; ++k)
    for (int q = 0; q < 4; ++q) {
      T acc = T(0);
#pragma unroll
      for (int col = 0; col < M; ++col) acc = m_fma(K[dlqr_kidx_m<M>(env, D, j, q, M * k + col)], se[k][col], acc);
      u[q] -= acc;
    }
}

// The CE phase of fedCE_iteration (:199-223) / do_control with 'dlqr' (:297-329): trajectory sample -> error_state9 against
// [0, 0, yaw, vel, pos] -> u = -K e (coupled over the env's drones) + (M G, 0, 0, 0) -> the ThrustOmega low level on the uncapped u
// (cap_u touches only the returned u, :223-231) -> the step (wind from Consts), n_steps steps in one launch, state and PID memory in
// registers.  256 / D whole envs per workgroup.  obs_log [T,n,20] / obs_last [n,20] may be NULL.
template <typename T, typename S, bool DRAG>
__global__ __launch_bounds__(kFedceBlock) void k_dlqr_omega_rollout(const Consts<T> c, const T* __restrict__ K, const int E, const int D,
                                                                    const size_t ld, double t, const double ctrl_dt, const int n_steps,
                                                                    const int traj_mode, S* __restrict__ state,
                                                                    const T* __restrict__ origin, const T* __restrict__ lem,
                                                                    const SegTable segs, const int* __restrict__ tinfo,
                                                                    T* __restrict__ last_rpm, T* __restrict__ ll,
                                                                    S* __restrict__ obs_log, S* __restrict__ obs_last) {
  constexpr int M = kOmegaM;
  __shared__ T se[kFedceBlock][M];
  const int epb = kFedceBlock / D;
  const int le = threadIdx.x / D, j = threadIdx.x - le * D;
  const size_t env = (size_t)blockIdx.x * epb + le;
  const bool valid = le < epb && env < (size_t)E;
  const int n = E * D;
  const size_t i = env * D + j;
  State<T> s;
  V3<T> org = {T(0), T(0), T(0)};
  LemniscateParams<T> P = {};
  TrajInfo ti = {0, 1, 0, 0};
  T prev[4] = {T(0), T(0), T(0), T(0)}, clipped[4] = {T(0), T(0), T(0), T(0)};
  LowLevelState<T> L;
  L.last_omega = L.integral = {T(0), T(0), T(0)};
  if (valid) {
    load_state<S, T>(state, ld, i, s);
    org = load_origin(origin, ld, i);
    load_traj(traj_mode, lem, tinfo, ld, i, P, ti);
    load_prev_rpm<DRAG>(last_rpm, ld, i, prev);
    L = load_lowlevel(ll, ld, i);
  }
  const T(*my_env)[M] = se + le * D;
  for (int step = 0; step < n_steps; ++step) {
    if (valid) {
      const Desired<T> des = sample_traj(traj_mode, P, segs, ti, t, org);
      T e[M];
      error_state9<T>(euler_from_quat(s.q), s.v, s.p - des.p, des.v, des.yaw, e);
      for (int k = 0; k < M; ++k) se[threadIdx.x][k] = e[k];
    }
    __syncthreads();
    if (valid) {
      T u[4], act[4];
      dlqr_input_m<T, M>(K, env, D, j, my_env, u);
      u[0] += c.gravity;
      thrust_omega_control(c, (T)ctrl_dt, u, s.w, L, act);
      aviary_step<T, false, DRAG>(c, s, act, prev, clipped);
      if (obs_log || (obs_last && step == n_steps - 1)) {
        T o[kObsDim];
        pack_obs(s, org, clipped, o);
        if (obs_log)
          for (int k = 0; k < 5; ++k) store4<S, T>(obs_log + ((size_t)step * n + i) * kObsDim + 4 * k, o + 4 * k);
        if (obs_last && step == n_steps - 1)
          for (int k = 0; k < 5; ++k) store4<S, T>(obs_last + i * kObsDim + 4 * k, o + 4 * k);
      }
    }
    __syncthreads();
    t += ctrl_dt;
  }
  if (valid) {
    store_state<S, T>(state, ld, i, s);
    store_lowlevel(ll, ld, i, L);
    if (last_rpm && n_steps > 0) store_last_rpm<DRAG>(last_rpm, ld, i, DRAG ? prev : clipped);
  }
}

// DecentralizedLQROmega.compute(obs, skip_low_level) for every env (:212-231): obs [n,20], des [n,11] (pos, vel, -, yaw, -) ->
// u [n,4] = cap_u(the drone's slice of -K e + (M G, 0, 0, 0)); action [n,4] = compute_low_level(uncapped u, obs), which advances the PID
// memory in ll -- act_out NULL is skip_low_level: ll is not touched.
template <typename T, typename S>
__global__ __launch_bounds__(kFedceBlock) void k_dlqr_omega_compute(const Consts<T> c, const T* __restrict__ K, const int E, const int D,
                                                                    const size_t ld, const T ctrl_dt, T* __restrict__ ll,
                                                                    const S* __restrict__ obs, const S* __restrict__ des,
                                                                    S* __restrict__ u_out, S* __restrict__ act_out) {
  constexpr int M = kOmegaM;
  __shared__ T se[kFedceBlock][M];
  const int epb = kFedceBlock / D;
  const int le = threadIdx.x / D, j = threadIdx.x - le * D;
  const size_t env = (size_t)blockIdx.x * epb + le;
  const bool valid = le < epb && env < (size_t)E;
  const size_t i = env * D + j;
  if (valid) {
    const S* o = obs + i * kObsDim;
    const S* d = des + i * 11;
    T e[M];
    const V3<T> perr = {(T)o[0] - (T)d[0], (T)o[1] - (T)d[1], (T)o[2] - (T)d[2]};
    error_state9<T>(obs_rpy<T>(o), obs_vel<T>(o), perr, V3<T>{(T)d[3], (T)d[4], (T)d[5]}, (T)d[9], e);
    for (int k = 0; k < M; ++k) se[threadIdx.x][k] = e[k];
  }
  __syncthreads();
  if (valid) {
    T u[4], act[4];
    dlqr_input_m<T, M>(K, env, D, j, se + le * D, u);
    u[0] += c.gravity;
    if (act_out) {
      const S* o = obs + i * kObsDim;
      const T q[4] = {(T)o[3], (T)o[4], (T)o[5], (T)o[6]};
      const V3<T> cur = mulT(quat_to_rot(q), obs_ang_vel<T>(o));
      LowLevelState<T> L = load_lowlevel(ll, ld, i);
      thrust_omega_control(c, ctrl_dt, u, cur, L, act);
      store_lowlevel(ll, ld, i, L);
      store4<S, T>(act_out + i * 4, act);
    }
    if (u_out) {
      u[0] = m_clamp(u[0], T(4) * c.min_motor_thrust, c.max_motor_thrust);       // cap_u (:233-236), after the action is made
      store4<S, T>(u_out + i * 4, u);
    }
  }
}

// The nominal controller of the CBF-filtered step with 'dlqr' (simulations/CBFTest.py:303-343): ctrl[0].compute(obs, skip_low_level=True)
// for the envs [e0, e_end) from the state planes (Lemniscates only, like every nominal of that step).  Per drone: trajectory sample ->
// error_state9 against [0, 0, yaw, vel, pos] -> u = -sum_k K e_k in drone order + (M G, 0, 0, 0) -> cap_u, whose output is what the script
// feeds the filter (:323-324, unlike the unfiltered loop's low level) -> u_hat = (u0 - hover_sub, u1..3) [n,4] and xdes [n,9] into the
// scratch planes the QP and k_lowlevel_step read.  The layout is k_dlqr_omega_rollout's: 256 / D whole envs per workgroup.
template <typename T, typename S>
__global__ __launch_bounds__(kFedceBlock) void k_cbf_nominal_dlqr_omega(const Consts<T> c, const T* __restrict__ K, const int e0,
                                                                        const int e_end, const int D, const size_t ld, const double t,
                                                                        const T hover_sub, const S* __restrict__ state,
                                                                        const T* __restrict__ lem, S* __restrict__ unom,
                                                                        S* __restrict__ xdes) {
  constexpr int M = kOmegaM;
  __shared__ T se[kFedceBlock][M];
  const int epb = kFedceBlock / D;
  const int le = threadIdx.x / D, j = threadIdx.x - le * D;
  const size_t env = (size_t)e0 + (size_t)blockIdx.x * epb + le;
  const bool valid = le < epb && env < (size_t)e_end;
  const size_t i = env * D + j;
  Desired<T> des = {};
  LemniscateParams<T> P = {};
  if (valid) {
    State<T> s;
    load_state<S, T>(state, ld, i, s);
    P = load_lemniscate(lem, ld, i);
    des = lemniscate_local(P, t);
    T e[M];
    error_state9<T>(euler_from_quat(s.q), s.v, s.p - des.p, des.v, des.yaw, e);
    for (int k = 0; k < M; ++k) se[threadIdx.x][k] = e[k];
  }
  __syncthreads();
  if (valid) {
    T u[4];
    dlqr_input_m<T, M>(K, env, D, j, se + le * D, u);
    u[0] += c.gravity;
    u[0] = m_clamp(u[0], T(4) * c.min_motor_thrust, c.max_motor_thrust);         // cap_u (:233-236)
    u[0] -= hover_sub;
    store4<S, T>(unom + i * 4, u);
    S* xd = xdes + i * 9;
    xd[0] = (S)0; xd[1] = (S)0; xd[2] = (S)des.yaw;
    xd[3] = (S)des.v.x; xd[4] = (S)des.v.y; xd[5] = (S)des.v.z;
    xd[6] = (S)(des.p.x + P.cx); xd[7] = (S)(des.p.y + P.cy); xd[8] = (S)(des.p.z + P.cz);
  }
}

}  // namespace mds
