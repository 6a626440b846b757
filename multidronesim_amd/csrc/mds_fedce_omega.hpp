// The arithmetic of the thrust / body-rate FedCE learner (control/dlqr/decentralized_lqr_omega.py, DecentralizedLQROmega), as
// templates on the scalar type and on the model's dimensions (M states, N inputs, M + N regressors: 9, 4, 13 here; the 10-state
// yank learner can instantiate the same code).  Host-compilable like mds_math.hpp: HIP-only constructs sit behind __HIPCC__.
//
//   error_state9 : DecentralizedLQROmega.error_state (:174-183) on x = obs_to_lin_model(obs, 9) = [rpy, vel, pos].
//   rk45_linear  : forward_predict (:87-97) -- scipy.integrate.solve_ivp's default method (RK45, rtol 1e-3, atol 1e-6) on an
//                  autonomous right-hand side, restated from the published algorithm (Hairer, Norsett, Wanner, "Solving Ordinary
//                  Differential Equations I", II.4 for the first step; Dormand & Prince 1980 for the 5(4) pair; the step control
//                  as scipy 1.15 documents it: RMS norm of err / (atol + rtol max(|y|, |y_new|)), safety 0.9, factors in
//                  [0.2, 10], no growth right after a rejected step, the last step clipped to the bound).
//   rls2_update  : theta_update2 (:110-123) for one drone with W = V^-1 carried beside V by Sherman-Morrison.
#pragma once
#include "mds_math.hpp"

namespace mds {

// (roll, pitch, wrapped yaw error, R_eq^T (vel - vel_des), R_eq^T pos_err), R_eq = Rz(yaw_des): the rotation part is what
// lqr_omega_control / lqr12_error do (R_eq^T R(rpy) = Rz(yaw - yaw_des) Ry Rx).
template <typename T>
MDS_HD void error_state9(V3<T> rpy, V3<T> vel, V3<T> pos_err, V3<T> vel_des, T yaw_des, T e[9]) {
  e[0] = rpy.x;
  e[1] = rpy.y;
  const T dy = rpy.z - yaw_des;
  e[2] = m_fma(T(-6.283185307179586476925), m_rint(dy * T(0.15915494309189533577)), dy);
  T sy, cy;
  m_sincos(reduced_phase<T>(0.0, T(0), yaw_des), &sy, &cy);
  const V3<T> dv = vel - vel_des, dp = pos_err;
  e[3] = cy * dv.x + sy * dv.y; e[4] = -sy * dv.x + cy * dv.y; e[5] = dv.z;
  e[6] = cy * dp.x + sy * dp.y; e[7] = -sy * dp.x + cy * dp.y; e[8] = dp.z;
}

// ---- rk45_linear ----------------------------------------------------------------------------------------------------------
// status bits of rk45_linear (0: the bound was reached); any bit set means y is not to be used
constexpr int kRk45Cap = 1;          // kRk45MaxAttempts step attempts did not reach the bound
constexpr int kRk45NonFinite = 2;    // a norm or a step size was not finite
constexpr int kRk45TooSmall = 4;     // solve_ivp's own failure: the step fell below 10 ulp(t)
constexpr int kRk45MaxAttempts = 16; // (the reference's loop: 1 to 3 attempts per call)

template <typename T> MDS_HD bool rk_finite(T x) { return (x - x) == T(0); }       // false for NaN and +-inf
MDS_HD double rk_pow(double x, double p) { return pow(x, p); }
MDS_HD float rk_pow(float x, float p) { return powf(x, p); }
MDS_HD double rk_ulp10(double t) { return 10.0 * (nextafter(t, INFINITY) - t); }
MDS_HD float rk_ulp10(float t) { return 10.0f * (nextafterf(t, INFINITY) - t); }

template <typename T, int M> MDS_HD T rk_rms(const T v[M], const T scale[M]) {
  T ss = T(0);
  for (int k = 0; k < M; ++k) {
    const T q = v[k] / scale[k];
    ss += q * q;
  }
  return m_sqrt(ss / T(M));
}

// y(tb) of y' = f(y), y(0) = y0; f(y, dy) is any callable (one thread with the whole matrix on the host, a 16-lane row with a
// butterfly sum in the identification kernel: every lane of the row then takes the same decisions from the same bits).
// Returns the status; *steps = accepted steps, *nfev = right-hand-side evaluations (as solve_ivp counts them).
template <typename T, int M, typename RHS>
MDS_HD int rk45_linear(const RHS& f, const T y0[M], T tb, T rtol, T atol, T y[M], int* steps, int* nfev) {
  T K[7][M], scale[M], tmp[M], ynew[M];
  int nf = 0, acc = 0;
  for (int k = 0; k < M; ++k) y[k] = y0[k];
  f(y, K[0]);
  ++nf;
  // select_initial_step (order 4)
  T h_abs;
  {
    for (int k = 0; k < M; ++k) scale[k] = atol + m_abs(y[k]) * rtol;
    const T d0 = rk_rms<T, M>(y, scale), d1 = rk_rms<T, M>(K[0], scale);
    T h0 = (d0 < T(1e-5) || d1 < T(1e-5)) ? T(1e-6) : T(0.01) * d0 / d1;
    h0 = m_min(h0, tb);
    for (int k = 0; k < M; ++k) tmp[k] = y[k] + h0 * K[0][k];
    f(tmp, K[1]);
    ++nf;
    for (int k = 0; k < M; ++k) tmp[k] = K[1][k] - K[0][k];
    const T d2 = rk_rms<T, M>(tmp, scale) / h0;
    const T h1 = (d1 <= T(1e-15) && d2 <= T(1e-15)) ? m_max(T(1e-6), h0 * T(1e-3)) : rk_pow(T(0.01) / m_max(d1, d2), T(0.2));
    h_abs = m_min(m_min(T(100) * h0, h1), tb);
    if (!rk_finite(d0) || !rk_finite(d1) || !rk_finite(d2) || !rk_finite(h_abs)) {
      *steps = 0; *nfev = nf;
      return kRk45NonFinite;
    }
  }
  T t = T(0);
  bool rejected = false;          // of the current step: cleared when a step is accepted (scipy's step_rejected)
  int status = kRk45Cap;
  for (int attempt = 0; attempt < kRk45MaxAttempts; ++attempt) {
    const T min_step = rk_ulp10(t);
    if (!rejected && h_abs < min_step) h_abs = min_step;       // the clamp at the top of _step_impl
    if (h_abs < min_step) { status = kRk45TooSmall; break; }
    T t_new = t + h_abs;
    if (t_new - tb > T(0)) t_new = tb;
    const T h = t_new - t;
    h_abs = m_abs(h);
    // Dormand-Prince 5(4) stages (FSAL: K[0] is f(y))
    for (int k = 0; k < M; ++k) tmp[k] = y[k] + (K[0][k] * T(1.0 / 5.0)) * h;
    f(tmp, K[1]);
    for (int k = 0; k < M; ++k) tmp[k] = y[k] + (K[0][k] * T(3.0 / 40.0) + K[1][k] * T(9.0 / 40.0)) * h;
    f(tmp, K[2]);
    for (int k = 0; k < M; ++k) tmp[k] = y[k] + (K[0][k] * T(44.0 / 45.0) + K[1][k] * T(-56.0 / 15.0) + K[2][k] * T(32.0 / 9.0)) * h;
    f(tmp, K[3]);
    for (int k = 0; k < M; ++k)
      tmp[k] = y[k] + (K[0][k] * T(19372.0 / 6561.0) + K[1][k] * T(-25360.0 / 2187.0) + K[2][k] * T(64448.0 / 6561.0) +
                       K[3][k] * T(-212.0 / 729.0)) * h;
    f(tmp, K[4]);
    for (int k = 0; k < M; ++k)
      tmp[k] = y[k] + (K[0][k] * T(9017.0 / 3168.0) + K[1][k] * T(-355.0 / 33.0) + K[2][k] * T(46732.0 / 5247.0) +
                       K[3][k] * T(49.0 / 176.0) + K[4][k] * T(-5103.0 / 18656.0)) * h;
    f(tmp, K[5]);
    for (int k = 0; k < M; ++k)
      ynew[k] = y[k] + h * (K[0][k] * T(35.0 / 384.0) + K[2][k] * T(500.0 / 1113.0) + K[3][k] * T(125.0 / 192.0) +
                            K[4][k] * T(-2187.0 / 6784.0) + K[5][k] * T(11.0 / 84.0));
    f(ynew, K[6]);
    nf += 6;
    for (int k = 0; k < M; ++k) {
      scale[k] = atol + m_max(m_abs(y[k]), m_abs(ynew[k])) * rtol;
      tmp[k] = (K[0][k] * T(-71.0 / 57600.0) + K[2][k] * T(71.0 / 16695.0) + K[3][k] * T(-71.0 / 1920.0) +
                K[4][k] * T(17253.0 / 339200.0) + K[5][k] * T(-22.0 / 525.0) + K[6][k] * T(1.0 / 40.0)) * h;
    }
    const T en = rk_rms<T, M>(tmp, scale);
    if (!rk_finite(en)) { status = kRk45NonFinite; break; }    // a failure, not a rejected step: NaN compares false both ways
    if (en < T(1)) {
      T factor = en == T(0) ? T(10) : m_min(T(10), T(0.9) * rk_pow(en, T(-0.2)));
      if (rejected) factor = m_min(T(1), factor);
      h_abs *= factor;
      rejected = false;
      ++acc;
      t = t_new;
      for (int k = 0; k < M; ++k) { y[k] = ynew[k]; K[0][k] = K[6][k]; }
      if (t - tb >= T(0)) { status = 0; break; }
    } else {
      h_abs *= m_max(T(0.2), T(0.9) * rk_pow(en, T(-0.2)));
      rejected = true;
    }
  }
  *steps = acc;
  *nfev = nf;
  return status;
}

// f(e) = theta^T [e; u] with the whole theta [(M + N), M] (row-major) in one thread: Ahat e + Bhat u of forward_predict
template <typename T, int M, int N> struct LinearRhs {
  const T* theta;
  const T* u;
  MDS_HD void operator()(const T y[M], T dy[M]) const {
    for (int c = 0; c < M; ++c) {
      T a = T(0);
      for (int r = 0; r < M; ++r) a = m_fma(theta[r * M + c], y[r], a);
      for (int r = 0; r < N; ++r) a = m_fma(theta[(M + r) * M + c], u[r], a);
      dy[c] = a;
    }
  }
};

// ---- rls2_update ----------------------------------------------------------------------------------------------------------
// theta_update2 for one drone, one thread: pred = forward_predict(x_tp1, phi[M:]) (sic: from x_tp1, :119),
// theta <- theta + V^-1 phi (x_tp1^T - pred^T) with theta and V taken before the update, then V <- V + phi phi^T.  W = V^-1 is
// carried: g = W phi, W <- W - g g^T / (1 + phi^T g).  Returns rk45_linear's status; non-zero leaves theta, V and W as they were.
template <typename T, int M, int N>
MDS_HD int rls2_update(T* theta, T* V, T* W, const T* phi, const T* xtp1, T ctrl_dt, int* steps, int* nfev) {
  constexpr int R = M + N;
  T pred[M], g[R];
  const LinearRhs<T, M, N> f = {theta, phi + M};
  const int st = rk45_linear<T, M>(f, xtp1, ctrl_dt, T(1e-3), T(1e-6), pred, steps, nfev);
  if (st) return st;
  T s = T(1);
  for (int r = 0; r < R; ++r) {
    T a = T(0);
    for (int k = 0; k < R; ++k) a = m_fma(W[r * R + k], phi[k], a);
    g[r] = a;
  }
  for (int r = 0; r < R; ++r) s = m_fma(phi[r], g[r], s);
  for (int r = 0; r < R; ++r) {
    for (int c = 0; c < M; ++c) theta[r * M + c] = m_fma(g[r], xtp1[c] - pred[c], theta[r * M + c]);
    for (int k = 0; k < R; ++k) {
      W[r * R + k] -= g[r] * (g[k] / s);
      V[r * R + k] = m_fma(phi[r], phi[k], V[r * R + k]);
    }
  }
  return 0;
}

// ---- rls_cov_update -------------------------------------------------------------------------------------------------------
// theta_update (:125-139), the covariance form, for one drone, one thread.  Here the reference's P is W: L = W phi / (1 + phi^T W phi),
// theta <- theta + L (x_tp1^T - pred^T), W <- (I - L phi^T) W = W - L (phi^T W) with theta and W taken before the update.  phi^T W is
// the column sum, not (W phi)^T: the reference does not symmetrise.  V <- V + phi phi^T keeps (V, W) an inverse pair.  Returns
// rk45_linear's status; non-zero leaves theta, V and W as they were.
template <typename T, int M, int N>
MDS_HD int rls_cov_update(T* theta, T* V, T* W, const T* phi, const T* xtp1, T ctrl_dt, int* steps, int* nfev) {
  constexpr int R = M + N;
  T pred[M], g[R], pw[R];
  const LinearRhs<T, M, N> f = {theta, phi + M};
  const int st = rk45_linear<T, M>(f, xtp1, ctrl_dt, T(1e-3), T(1e-6), pred, steps, nfev);
  if (st) return st;
  T s = T(1);
  for (int r = 0; r < R; ++r) {
    T a = T(0), b = T(0);
    for (int k = 0; k < R; ++k) {
      a = m_fma(W[r * R + k], phi[k], a);
      b = m_fma(phi[k], W[k * R + r], b);
    }
    g[r] = a;
    pw[r] = b;
  }
  for (int r = 0; r < R; ++r) s = m_fma(phi[r], g[r], s);
  for (int r = 0; r < R; ++r) {
    const T l = g[r] / s;
    for (int c = 0; c < M; ++c) theta[r * M + c] = m_fma(l, xtp1[c] - pred[c], theta[r * M + c]);
    for (int k = 0; k < R; ++k) {
      W[r * R + k] -= l * pw[k];
      V[r * R + k] = m_fma(phi[r], phi[k], V[r * R + k]);
    }
  }
  return 0;
}

#if defined(__HIPCC__)
// The same update with lane r of a 16-lane row owning row r of theta, V and W (rows R..15 hold zeros and stay zero).  row_sum is the
// row's butterfly sum; phir = phi[r] (0 on the idle lanes), innov = x_tp1 - pred (the same on every lane).
template <int M, int N, typename SUM>
__device__ __forceinline__ void rls2_update_row(const SUM& row_sum, double phir, const double* phi, const double* innov, double* th_row,
                                                double* V_row, double* W_row) {
  constexpr int R = M + N;
  double g = 0.0;
#pragma unroll
  for (int k = 0; k < R; ++k) g = fma(W_row[k], phi[k], g);
  const double s = 1.0 + row_sum(phir * g);
#pragma unroll
  for (int c = 0; c < M; ++c) th_row[c] = fma(g, innov[c], th_row[c]);
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const double gk = __shfl(g, k, 16);
    W_row[k] -= g * (gk / s);
    V_row[k] = fma(phir, phi[k], V_row[k]);
  }
}

// rls_cov_update with the same split: lane r owns row r of theta, V and W (the reference's P).  (W phi)_r is local, phi^T W phi one
// butterfly sum, (phi^T W)_c a column sum over the lanes (R butterflies; the idle lanes add zeros).
template <int M, int N, typename SUM>
__device__ __forceinline__ void rls_cov_update_row(const SUM& row_sum, double phir, const double* phi, const double* innov, double* th_row,
                                                   double* V_row, double* W_row) {
  constexpr int R = M + N;
  double g = 0.0;
#pragma unroll
  for (int k = 0; k < R; ++k) g = fma(W_row[k], phi[k], g);
  const double l = g / (1.0 + row_sum(phir * g));
#pragma unroll
  for (int c = 0; c < M; ++c) th_row[c] = fma(l, innov[c], th_row[c]);
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const double pw = row_sum(phir * W_row[k]);
    W_row[k] -= l * pw;
    V_row[k] = fma(phir, phi[k], V_row[k]);
  }
}
#endif

}  // namespace mds
