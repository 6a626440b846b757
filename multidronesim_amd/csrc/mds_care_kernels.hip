// The dLQR gains of both FedCE models on the device: one continuous Riccati equation per (env, group of drones), float64
// (DecentralizedLQR / DecentralizedLQROmega.compute_controller; the arithmetic is mds_care.hpp).  Included by
// mds_api.hip in part 2 only, after the FedCE kernels.
//
//   k_care_solve<WIDTH> : one wavefront per problem, lane c owns column c of the WIDTH x WIDTH Hamiltonian (18: one drone of the
//                         9-state model, 24: one drone of the 12-state model, 48: the xy-coupled pair of the 12-state model).  Both
//                         work matrices live in LDS as float64 with the odd row stride WIDTH + 1; the pivot search is a butterfly
//                         over the wave, the pivot row is the lane's own column entry and the multiplier column is read as an LDS
//                         broadcast.  A, B come straight from the learner state of the handle (theta), Q and R^-1 from the group
//                         table the host made of the caller's Q and R.  A solved problem writes its block of K_env [4D, MD]
//                         (float64); a failed one ors its status bits into status[env].
//   k_care_commit       : after every group of every env is done: an env without a status bit gets its K converted into the gain
//                         buffer the dLQR kernels read ([E][4][M D][D], the env's storage type); an env with one keeps its previous
//                         gain entirely and its float64 K is zeroed.
#include <hip/hip_runtime.h>

#include "mds_care.hpp"

namespace mds {

template <int WIDTH> struct CareShape;
template <> struct CareShape<18> { static constexpr int M = 9, ND = 1, WAVES = 4; };
template <> struct CareShape<24> { static constexpr int M = 12, ND = 1, WAVES = 4; };
template <> struct CareShape<48> { static constexpr int M = 12, ND = 2, WAVES = 1; };     // 43 KiB of LDS per problem

// The drones of every group of one size class (singles or pairs), by value in the kernel arguments
struct CareGroups {
  int count;
  int drone[kFedceMaxD][2];
};

// column c of lane c; every phase ends with the wavefront's LDS barrier
struct CareWave {
  int lane;
  template <typename F> __device__ __forceinline__ void cols(int n, const F& f) const {
    if (lane < n) f(lane);
    wave_lds_sync();
  }
  template <typename F> __device__ __forceinline__ double max(int n, const F& f) const {
    double v = lane < n ? f(lane) : 0.0;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
      const double o = __shfl_xor(v, s, 64);
      v = (o > v || o != o) ? o : v;
    }
    return v;
  }
  template <typename F> __device__ __forceinline__ int argmax(int lo, int n, const F& f) const {
    double v = (lane >= lo && lane < n) ? f(lane) : -1.0;       // f >= 0 on the live lanes; a NaN never wins, as in CareSerial
    int at = lane;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
      const double ov = __shfl_xor(v, s, 64);
      const int oa = __shfl_xor(at, s, 64);
      const bool take = ov > v || (ov == v && oa < at);
      v = take ? ov : v;
      at = take ? oa : at;
    }
    return (at >= lo && at < n) ? at : lo;                        // every live lane held a NaN: CareSerial's answer
  }
};

template <int WIDTH>
__global__ __launch_bounds__(64 * CareShape<WIDTH>::WAVES) void k_care_solve(const int E, const int D, const CareGroups groups,
                                                                             const double* __restrict__ theta,
                                                                             const double* __restrict__ Rinv_tab,
                                                                             const double* __restrict__ Q_tab, const int max_iter,
                                                                             double* __restrict__ K64, int32_t* __restrict__ status,
                                                                             int32_t* __restrict__ iters_out) {
  using S = CareShape<WIDTH>;
  constexpr int M = S::M, ND = S::ND, NS = M * ND, NU = 4 * ND, WAVES = S::WAVES;
  constexpr int TH = M == 12 ? 12 : 13 * 9;         // doubles of one drone's learner state
  __shared__ CareWork<NS> work[WAVES];
  __shared__ double sA[WAVES][NS * NS], sB[WAVES][NS * NU], sR[WAVES][NU * NU];
  const int wave = threadIdx.x >> 6;
  const CareWave x = {(int)(threadIdx.x & 63)};
  const long prob = (long)blockIdx.x * WAVES + wave;
  if (prob >= (long)E * groups.count) return;       // whole wavefronts leave
  const int env = (int)(prob / groups.count), g = (int)(prob - (long)env * groups.count);
  double* A = sA[wave];
  double* B = sB[wave];
  double* Ri = sR[wave];
  // stage the group's model: block-diagonal A, B and R^-1 over its drones
  for (int k = x.lane; k < NS * NS; k += 64) {
    const int i = k / NS, j = k - i * NS, a = i / M, b = j / M;
    const double* th = theta + ((size_t)env * D + groups.drone[g][a]) * TH;
    A[k] = a != b ? 0.0 : (M == 12 ? care_model12_A(th, i - a * M, j - b * M) : care_model9_A(th, i - a * M, j - b * M));
  }
  for (int k = x.lane; k < NS * NU; k += 64) {
    const int i = k / NU, q = k - i * NU, a = i / M, b = q / 4;
    const double* th = theta + ((size_t)env * D + groups.drone[g][a]) * TH;
    B[k] = a != b ? 0.0 : (M == 12 ? care_model12_B(th, i - a * M, q - 4 * b) : care_model9_B(th, i - a * M, q - 4 * b));
  }
  for (int k = x.lane; k < NU * NU; k += 64) {
    const int q = k / NU, r = k - q * NU, a = q / 4, b = r / 4;
    Ri[k] = a != b ? 0.0 : Rinv_tab[(size_t)groups.drone[g][a] * 16 + (q - 4 * a) * 4 + (r - 4 * b)];
  }
  wave_lds_sync();
  const double* Q = Q_tab + (size_t)g * NS * NS;
  int it = 0;
  double res;
  const int st = care_solve<NS, NU>(x, A, B, Ri, Q, work[wave], max_iter, &it, &res);
  if (st == 0) {
    const size_t row = (size_t)M * D;
    double* Ke = K64 + (size_t)env * 4 * D * row;
    care_gain<NS, NU>(x, B, Ri, work[wave], [&](int q, int j, double v) {
      const int a = q >> 2, b = j / M;
      Ke[((size_t)4 * groups.drone[g][a] + (q & 3)) * row + (size_t)M * groups.drone[g][b] + (j - b * M)] = v;
    });
  }
  if (x.lane == 0) {
    if (st) atomicOr(status + env, st);
    if (iters_out) atomicMax(iters_out + env, it);
  }
}

// K64 [E, 4D, MD] -> the gain buffer [E][4][M D][D] in T for the envs without a status bit; the others keep theirs and lose their K64
template <typename T, int M>
__global__ __launch_bounds__(256) void k_care_commit(const int E, const int D, double* __restrict__ K64, const int32_t* __restrict__ status,
                                                     T* __restrict__ gain) {
  const size_t per = (size_t)4 * D * M * D;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= per * (size_t)E) return;
  const size_t env = idx / per, k = idx - env * per;
  const int r = (int)(k / ((size_t)M * D)), col = (int)(k - (size_t)r * M * D);
  if (status[env] == 0)
    gain[dlqr_kidx_m<M>(env, D, r >> 2, r & 3, col)] = (T)K64[idx];
  else
    K64[idx] = 0.0;
}

}  // namespace mds
