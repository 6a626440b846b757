// FedCE system identification and the decentralised LQR (control/dlqr/decentralized_lqr.py, simulations/EnvGeometric.py
// fedCE / fedCE_iteration).  Included by mds_api.hip in part 2 only (DESIGN.md "FedCE").
//
//   k_fedce_identify : one warm-up or exploration phase (T steps) per launch.  16 lanes per drone: lane r keeps row r of the
//                      RLS covariance P (float64, 16 values) in registers for the whole phase; the 12 free entries of the
//                      drone's theta (float64) are replicated on its 16 lanes, the physics is replicated too (every lane steps
//                      the same state, lane 0 stores it).  P phi is one dot product per lane; phi^T P phi and the 16 columns of
//                      phi^T P are butterfly sums inside the 16-lane row (__shfl_xor), so P never crosses HBM inside a phase.
//   k_dlqr_rollout   : one CE phase / do_control run per launch, one drone per lane, whole envs per workgroup: the error
//                      states of an env's D drones are exchanged through LDS every step and each drone's 4 inputs come from
//                      its rows of the env's own gain K [4D, 12D] (layout in dlqr_kidx: the D drones of an env read
//                      consecutive addresses).
//   k_dlqr_compute   : DecentralizedLQR.compute(obs) for every env, one call.
#include <hip/hip_runtime.h>

#include "mds_math.hpp"
#include "mds_traj.hpp"

namespace mds {

constexpr int kFedceMaxD = 16;     // drones per env of the dLQR kernels (one env's gain rows, LDS exchange)
constexpr int kFedceBlock = 256;   // 16 drones per workgroup in k_fedce_identify; 256 / D whole envs in the dLQR kernels

// The free entries of one drone's theta = [A^T; B^T] (16 x 12, DecentralizedLQR.project_theta):
//   f[0] = A[6,1] = theta[1][6], f[1] = A[7,0] = theta[0][7], f[2 + 3a + b] = B[3+a, 1+b] = theta[13+b][3+a], f[11] = B[8,0] = theta[12][8].
// The fixed ones are A[0:3,3:6] = A[9:12,6:9] = I; every other entry is 0.
struct FedceModel {
  double mg;         // M G: the hover thrust taken off u[0] in phi
  double g, mass;    // the true model (LinearizedModel.A / B) of the second pred_errors entry
  double J[3];
  double ctrl_dt;    // CTRL_TIMESTEP of est_x_dot
};

// theta^T phi with the projected theta (the 12 predictions x_dot_hat of DecentralizedLQR.approx_theta_update)
__device__ __forceinline__ void fedce_predict(const double f[12], const double phi[16], double y[12]) {
  y[0] = phi[3]; y[1] = phi[4]; y[2] = phi[5];
  for (int a = 0; a < 3; ++a) y[3 + a] = phi[13] * f[2 + 3 * a] + phi[14] * f[3 + 3 * a] + phi[15] * f[4 + 3 * a];
  y[6] = phi[1] * f[0];
  y[7] = phi[0] * f[1];
  y[8] = phi[12] * f[11];
  y[9] = phi[6]; y[10] = phi[7]; y[11] = phi[8];
}

// sum of v over the 16 lanes of this drone's row; every lane gets the same bits (butterfly: each node adds the same pair)
__device__ __forceinline__ double row_sum16(double v) {
  v += __shfl_xor(v, 8, 16);
  v += __shfl_xor(v, 4, 16);
  v += __shfl_xor(v, 2, 16);
  v += __shfl_xor(v, 1, 16);
  return v;
}

// LDS written by one lane and read by the other lanes of the same wavefront
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// DecentralizedLQR.approx_theta_update for one drone, lane r of its 16 (theta and P taken before the update):
//   L = P phi / (1 + phi^T P phi),  theta <- project(theta + L (x_dot^T - phi^T theta)),  P <- (I - L phi^T) P.
// phir = phi[r], read back from LDS (a register array indexed by the lane would live in scratch).
__device__ __forceinline__ void fedce_rls(double phir, double Prow[16], double f[12], const double phi[16], const double innov[12]) {
  double Pphi = 0.0;
#pragma unroll
  for (int k = 0; k < 16; ++k) Pphi = fma(Prow[k], phi[k], Pphi);
  const double s = 1.0 + row_sum16(phir * Pphi);
  const double L = Pphi / s;
  // w = phi^T P (row vector): the 16 column sums, each a butterfly over the row's lanes
#pragma unroll
  for (int c = 0; c < 16; ++c) Prow[c] -= L * row_sum16(phir * Prow[c]);
  // the free entries: rows 0, 1, 12..15 of theta
  const double L0 = __shfl(L, 0, 16), L1 = __shfl(L, 1, 16), L12 = __shfl(L, 12, 16);
  const double Lb[3] = {__shfl(L, 13, 16), __shfl(L, 14, 16), __shfl(L, 15, 16)};
  f[0] += L1 * innov[6];
  f[1] += L0 * innov[7];
#pragma unroll
  for (int a3 = 0; a3 < 3; ++a3)
#pragma unroll
    for (int b = 0; b < 3; ++b) f[2 + 3 * a3 + b] += Lb[b] * innov[3 + a3];
  f[11] += L12 * innov[8];
}

// x_des of fedCE_iteration as the error state reads it: yaw, yaw rate, velocity, position (x_des[2], [5], [6:9], [9:12])
struct FedceDes {
  double yaw, omega;
  V3<double> v, p;
};

// DecentralizedLQR.error_state(obs_to_lin_model(obs), x_des) in float64 from the state in the env's dtype (the obs' values)
template <typename T> __device__ __forceinline__ void fedce_error(const State<T>& s, V3<T> org, const FedceDes& xd, double e[12]) {
  const V3<T> rpy = euler_from_quat(s.q), av = quat_rotate(s.q, s.w);
  const V3<double> p = {(double)(s.p.x + org.x), (double)(s.p.y + org.y), (double)(s.p.z + org.z)};
  lqr12_error<double>(V3<double>{(double)rpy.x, (double)rpy.y, (double)rpy.z}, V3<double>{(double)av.x, (double)av.y, (double)av.z},
                      V3<double>{(double)s.v.x, (double)s.v.y, (double)s.v.z}, p - xd.p, xd.v, xd.yaw, xd.omega, e);
}

// One warm-up (u_mode 0: phi takes the raw input) or exploration phase (u_mode 1: phi takes action_to_input(input_to_action(u)))
// of fedCE_iteration for every drone, n_steps steps, wind from Consts.  Per step: e_t, phi = [e_t, u~ - (M G, 0, 0, 0)], the physics
// on input_to_action(u), e_{t+1}, x_dot = est_x_dot(e_{t+1}, phi), pred_errors, and (update != 0) the RLS update.
// u [T,n,4] float64; xdes [n,12] float64 (NULL: zeros); logs may be NULL: obs [T,n,20] S, pred_err [T,n,2], theta [T,n,12] float64.
template <typename T, typename S, bool DRAG>
__global__ __launch_bounds__(kFedceBlock) void k_fedce_identify(const Consts<T> c, const Consts<double> cd, const FedceModel fm, const int n,
                                                                const size_t ld, const int n_steps, S* __restrict__ state,
                                                                const T* __restrict__ origin, T* __restrict__ last_rpm,
                                                                const double* __restrict__ u_in, const int u_mode,
                                                                const double* __restrict__ xdes, const int update,
                                                                double* __restrict__ Pg, double* __restrict__ thg,
                                                                S* __restrict__ obs_log, double* __restrict__ perr_log,
                                                                double* __restrict__ theta_log) {
  __shared__ double sphi[kFedceBlock / 16][16];
  const int gid = blockIdx.x * kFedceBlock + threadIdx.x;
  const int i = gid >> 4, r = gid & 15;
  double* my_phi = sphi[threadIdx.x >> 4];
  if (i >= n) return;                        // whole 16-lane rows leave together
  State<T> s;
  load_state<S, T>(state, ld, i, s);
  const V3<T> org = load_origin(origin, ld, i);
  T prev[4] = {T(0), T(0), T(0), T(0)}, clipped[4] = {T(0), T(0), T(0), T(0)};
  // (the RPM planes in place here and at the end, not through load_prev_rpm / store_last_rpm as in k_fedce_omega_identify: with the
  // helpers this kernel's instructions come out in another order, and its assembly is pinned)
  if (DRAG)
    for (int k = 0; k < 4; ++k) prev[k] = last_rpm[k * ld + i];
  FedceDes xd = {0.0, 0.0, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
  if (xdes) {
    const double* x = xdes + (size_t)i * 12;
    xd = {x[2], x[5], {x[6], x[7], x[8]}, {x[9], x[10], x[11]}};
  }
  double Prow[16], f[12];
  for (int k = 0; k < 16; ++k) Prow[k] = Pg[((size_t)i * 16 + r) * 16 + k];
  for (int k = 0; k < 12; ++k) f[k] = thg[(size_t)i * 12 + k];
  double e[12];
  fedce_error<T>(s, org, xd, e);
  for (int t = 0; t < n_steps; ++t) {
    double u[4], act64[4], phi[16];
    const double* ut = u_in + ((size_t)t * n + i) * 4;
    for (int k = 0; k < 4; ++k) u[k] = ut[k];
    input_to_action<double>(cd, u, act64);
    for (int k = 0; k < 12; ++k) phi[k] = e[k];
    if (u_mode == 0) {
      phi[12] = fmax(u[0], 0.0) - fm.mg;     // input_to_action clips u[0] at 0 in place before u[0] -= M G
      phi[13] = u[1]; phi[14] = u[2]; phi[15] = u[3];
    } else {
      double ur[4];
      action_to_input<double>(cd, act64, 1, ur);
      phi[12] = ur[0] - fm.mg;
      phi[13] = ur[1]; phi[14] = ur[2]; phi[15] = ur[3];
    }
    const T act[4] = {(T)act64[0], (T)act64[1], (T)act64[2], (T)act64[3]};
    aviary_step<T, false, DRAG>(c, s, act, prev, clipped);
    double e1[12], xdot[12], y[12], innov[12];
    fedce_error<T>(s, org, xd, e1);
    for (int k = 0; k < 3; ++k) {            // est_x_dot
      xdot[k] = e1[3 + k];
      xdot[3 + k] = (e1[3 + k] - phi[3 + k]) / fm.ctrl_dt;
      xdot[6 + k] = (e1[6 + k] - phi[6 + k]) / fm.ctrl_dt;
      xdot[9 + k] = e1[6 + k];
    }
    fedce_predict(f, phi, y);
    for (int k = 0; k < 12; ++k) innov[k] = xdot[k] - y[k];
    if (perr_log && r < 2) {
      double ss = 0.0;
      if (r == 0) {
        for (int k = 0; k < 12; ++k) ss += innov[k] * innov[k];
      } else {                               // the true A, B (LinearizedModel.A / B)
        const double g[12] = {phi[3], phi[4], phi[5], phi[13] / fm.J[0], phi[14] / fm.J[1], phi[15] / fm.J[2],
                              phi[1] * fm.g, -(phi[0] * fm.g), phi[12] / fm.mass, phi[6], phi[7], phi[8]};
        for (int k = 0; k < 12; ++k) ss += (xdot[k] - g[k]) * (xdot[k] - g[k]);
      }
      perr_log[((size_t)t * n + i) * 2 + r] = sqrt(ss);
    }
    if (update) {
      if (r == 0)
        for (int k = 0; k < 16; ++k) my_phi[k] = phi[k];
      wave_lds_sync();
      const double phir = my_phi[r];
      wave_lds_sync();
      fedce_rls(phir, Prow, f, phi, innov);
    }
    if (theta_log && r == 0)
      for (int k = 0; k < 3; ++k) store4<double, double>(theta_log + ((size_t)t * n + i) * 12 + 4 * k, f + 4 * k);
    if (obs_log && r == 0) {
      T o[kObsDim];
      pack_obs(s, org, clipped, o);
      for (int k = 0; k < 5; ++k) store4<S, T>(obs_log + ((size_t)t * n + i) * kObsDim + 4 * k, o + 4 * k);
    }
    for (int k = 0; k < 12; ++k) e[k] = e1[k];
  }
  for (int k = 0; k < 16; ++k) Pg[((size_t)i * 16 + r) * 16 + k] = Prow[k];
  if (r == 0) {
    for (int k = 0; k < 3; ++k) store4<double, double>(thg + (size_t)i * 12 + 4 * k, f + 4 * k);
    store_state<S, T>(state, ld, i, s);
    if (last_rpm && n_steps > 0)
      for (int k = 0; k < 4; ++k) last_rpm[k * ld + i] = DRAG ? prev[k] : clipped[k];
  }
}

// Element of K_e[4j + q][12k + col] (env e's gain, row of drone j's input q, column of drone k's error col) in the device layout
// [E][4][12 D][D]: the D drones of an env read D consecutive elements for every (q, col).
__host__ __device__ __forceinline__ size_t dlqr_kidx(size_t env, int D, int j, int q, int col) {
  return ((env * 4 + (size_t)q) * (size_t)(12 * D) + (size_t)col) * (size_t)D + (size_t)j;
}

// u_j = -sum_k K_e[4j:4j+4, 12k:12k+12] e_k (DecentralizedLQR.compute, :326-342; the per-drone sums in the reference's order),
// e_k read from this env's slice of the LDS exchange buffer
template <typename T>
__device__ __forceinline__ void dlqr_input(const T* __restrict__ K, size_t env, int D, int j, const T (*se)[12], T u[4]) {
  for (int q = 0; q < 4; ++q) u[q] = T(0);
  for (int k = 0; k < D; ++k)
    for (int q = 0; q < 4; ++q) {
      T acc = T(0);
#pragma unroll
      for (int col = 0; col < 12; ++col) acc = m_fma(K[dlqr_kidx(env, D, j, q, 12 * k + col)], se[k][col], acc);
      u[q] -= acc;
    }
}

// The CE phase of fedCE_iteration / do_control with 'dlqr': trajectory sample -> error state -> u = -K e (coupled over the env's
// drones) + (M G, 0, 0, 0) -> input_to_action -> the step (wind from Consts), n_steps steps in one launch, state in registers.
// 256 / D whole envs per workgroup (drone i = env * D + j).  obs_log [T,n,20] / obs_last [n,20] may be NULL.
template <typename T, typename S, bool DRAG>
__global__ __launch_bounds__(kFedceBlock) void k_dlqr_rollout(const Consts<T> c, const T* __restrict__ K, const int E, const int D,
                                                              const size_t ld, double t, const double ctrl_dt, const int n_steps,
                                                              const int traj_mode, S* __restrict__ state,
                                                              const T* __restrict__ origin, const T* __restrict__ lem,
                                                              const SegTable segs, const int* __restrict__ tinfo,
                                                              T* __restrict__ last_rpm, S* __restrict__ obs_log,
                                                              S* __restrict__ obs_last) {
  __shared__ T se[kFedceBlock][12];
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
  if (valid) {
    load_state<S, T>(state, ld, i, s);
    org = load_origin(origin, ld, i);
    // (the trajectory and the RPM planes in place, not through load_traj / sample_traj / load_prev_rpm as in k_dlqr_omega_rollout: with the
    // helpers this kernel's and k_fedce_identify's instructions come out in another order, and their assembly is pinned)
    if (traj_mode == 1)
      P = {lem[lidx(0, i, ld)], lem[lidx(1, i, ld)], lem[lidx(2, i, ld)], lem[lidx(3, i, ld)], lem[lidx(4, i, ld)], lem[lidx(5, i, ld)],
           lem[lidx(6, i, ld)]};
    else
      ti = traj_info(tinfo, i);
    if (DRAG)
      for (int k = 0; k < 4; ++k) prev[k] = last_rpm[k * ld + i];
  }
  const T(*my_env)[12] = se + le * D;
  for (int step = 0; step < n_steps; ++step) {
    if (valid) {
      const Desired<T> des = traj_mode == 1 ? lemniscate_local(P, t) : TrajLocal<T>::eval(segs, ti, t, org);
      T e[12];
      lqr12_error<T>(euler_from_quat(s.q), quat_rotate(s.q, s.w), s.v, s.p - des.p, des.v, des.yaw, des.yaw_rate, e);
      for (int k = 0; k < 12; ++k) se[threadIdx.x][k] = e[k];
    }
    __syncthreads();
    if (valid) {
      T u[4], act[4];
      dlqr_input<T>(K, env, D, j, my_env, u);
      u[0] += c.gravity;
      input_to_action(c, u, act);
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
    if (last_rpm && n_steps > 0)
      for (int k = 0; k < 4; ++k) last_rpm[k * ld + i] = DRAG ? prev[k] : clipped[k];
  }
}

// DecentralizedLQR.compute(obs) for every env: obs [n,20], des [n,11] (pos, vel, -, yaw, omega) -> u [n,4] = the drone's slice of
// -K e (before the hover offset, as the reference returns it), action [n,4] = input_to_action(u + (M G, 0, 0, 0)).
template <typename T, typename S>
__global__ __launch_bounds__(kFedceBlock) void k_dlqr_compute(const Consts<T> c, const T* __restrict__ K, const int E, const int D,
                                                              const S* __restrict__ obs, const S* __restrict__ des,
                                                              S* __restrict__ u_out, S* __restrict__ act_out) {
  __shared__ T se[kFedceBlock][12];
  const int epb = kFedceBlock / D;
  const int le = threadIdx.x / D, j = threadIdx.x - le * D;
  const size_t env = (size_t)blockIdx.x * epb + le;
  const bool valid = le < epb && env < (size_t)E;
  const size_t i = env * D + j;
  if (valid) {
    const S* o = obs + i * kObsDim;
    const S* d = des + i * 11;
    T e[12];
    const V3<T> perr = {(T)o[0] - (T)d[0], (T)o[1] - (T)d[1], (T)o[2] - (T)d[2]};
    lqr12_error<T>(obs_rpy<T>(o), obs_ang_vel<T>(o), obs_vel<T>(o), perr, V3<T>{(T)d[3], (T)d[4], (T)d[5]}, (T)d[9], (T)d[10], e);
    for (int k = 0; k < 12; ++k) se[threadIdx.x][k] = e[k];
  }
  __syncthreads();
  if (valid) {
    T u[4], act[4];
    dlqr_input<T>(K, env, D, j, se + le * D, u);
    if (u_out) store4<S, T>(u_out + i * 4, u);
    u[0] += c.gravity;
    input_to_action(c, u, act);
    if (act_out) store4<S, T>(act_out + i * 4, act);
  }
}

}  // namespace mds
