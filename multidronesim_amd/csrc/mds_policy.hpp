// The MLP policy of the per-env episodes (include/mds.h mds_set_episode_policy): features, network, action -- the arithmetic stated
// once, templated on the compute type T like mds_episode.hpp.  The same header compiles with plain g++ (tests/episode_policy_main.cpp
// runs it against torch and the float64 oracle); nothing here is HIP-only, and it calls nothing but mds_math.hpp.
//
// Features x[12] of one drone, in T, from its state as pack_obs forms the observation columns:
//   x[0:3]  local position - local target          (the two operands of episode_reward_term)
//   x[3:6]  roll, pitch, yaw                       (observation columns 7:10)
//   x[6:9]  world velocity                         (columns 10:13)
//   x[9:12] world-frame angular velocity           (columns 13:16)
// ([UPSTREAM] the KIN observation, position relative to the target.)  There is no input-normalisation stage: an affine normaliser
// x' = (x - mu) / sigma folds into layer 1 on the host, W1' = W1 diag(1 / sigma), b1' = b1 - W1' mu, before the upload.
//
// Network: 1 or 2 hidden layers of one common width in 1..64, activation 0 = tanh | 1 = relu, a linear output of 4.  Weights packed as
// torch packs an nn.Sequential of Linear layers: weight [out][in] row-major, then bias [out], layer after layer
// (torch.cat([p.detach().flatten() for p in actor.parameters()])).
//
// Order of operations -- fixed here, so that another evaluation of the same chains (an MFMA form: v_mfma_f32_*_f32 computes a k-ordered
// fmaf chain) can reproduce this one to the bit: a neuron's pre-activation starts from its bias and takes
//   acc = m_fma(w[k], x[k], acc)       for k ascending,
// one chain per neuron, no tree.  Chains of different neurons are independent; in which order they are interleaved changes no bit.
//
// m_tanh(x): t = m_exp(-2 |x|), y = (1 - t) / (1 + t), with the sign of x.  (|y| <= 1, y(+-0) = +-0, y(+-inf) = +-1, NaN stays NaN;
// absolute error against float64 tanh: DESIGN.md.)
//
// Action: rpm[j] = rpm_base + rpm_scale * m_clamp(y[j], -1, 1), as one m_fma; defaults hover_rpm and 0.05 hover_rpm ([UPSTREAM]
// ActionType.RPM's pre-processing).  The motor clip is the step's own, as for a table action.
//
// Zero padding: the device code is instantiated for the widths of kPolicyWidths only; a narrower policy is uploaded zero-padded
// (policy_pad).  A padded hidden neuron has zero weights and bias, so it is act(0) = 0, and whatever reads it does
// m_fma(0, 0, acc) = acc: with finite weights and finite features the result is the unpadded one to the bit (finiteness of the weights
// is validated on upload).  policy_eval evaluates any width directly; policy_eval_w<W> is the fixed-width form the kernels use.
//
// fp16 storage is not built: the entry points refuse MDS_F16 handles until a storage-faithful oracle exists for the policy loop, as
// tests/fp16_oracle.py provides for the step.
#pragma once
#include "mds_math.hpp"

namespace mds {

constexpr int kPolicyIn = 12, kPolicyOut = 4, kPolicyMaxWidth = 64;
constexpr int kPolicyWidths[2] = {32, 64};           // the widths the device code is instantiated for
constexpr int kPolicyTanh = 0, kPolicyRelu = 1;

// number of weights of a policy (the length of the packed vector)
MDS_HD int policy_n_weights(int n_hidden, int width) {
  return (kPolicyIn + 1) * width + (n_hidden - 1) * (width + 1) * width + (width + 1) * kPolicyOut;
}
// the smallest instantiated width that holds `width`
inline int policy_device_width(int width) { return width <= kPolicyWidths[0] ? kPolicyWidths[0] : kPolicyWidths[1]; }

// src: a policy of `width` packed as above -> dst: the same policy of width W >= width, the new neurons' weights and biases zero
template <typename A, typename B> inline void policy_pad(const A* src, int n_hidden, int width, int W, B* dst) {
  for (int k = 0, n = policy_n_weights(n_hidden, W); k < n; ++k) dst[k] = B(0);
  int in = kPolicyIn, in_pad = kPolicyIn;
  for (int l = 0; l <= n_hidden; ++l) {
    const int out = l == n_hidden ? kPolicyOut : width, out_pad = l == n_hidden ? kPolicyOut : W;
    for (int j = 0; j < out; ++j)
      for (int k = 0; k < in; ++k) dst[j * in_pad + k] = (B)src[j * in + k];
    for (int j = 0; j < out; ++j) dst[out_pad * in_pad + j] = (B)src[out * in + j];
    src += (in + 1) * out;
    dst += (in_pad + 1) * out_pad;
    in = out;
    in_pad = out_pad;
  }
}

template <typename T> MDS_HD T m_tanh(T x) {
  const T t = m_exp(T(-2) * m_abs(x));
  const T y = (T(1) - t) / (T(1) + t);
  return x < T(0) ? -y : (x == T(0) ? x : y);          // (x == 0 returns x: the sign of a zero; a NaN x gives the NaN y)
}
template <typename T> MDS_HD T policy_act(int activation, T x) { return activation == kPolicyRelu ? (x > T(0) ? x : T(0)) : m_tanh(x); }
// N values in place, under one test of the (wave-uniform) activation
template <int N, typename T> MDS_HD void policy_act_n(int activation, T* v) {
  if (activation == kPolicyRelu) {
#if defined(__clang__)
#pragma unroll
#endif
    for (int j = 0; j < N; ++j) v[j] = v[j] > T(0) ? v[j] : T(0);
  } else {
#if defined(__clang__)
#pragma unroll
#endif
    for (int j = 0; j < N; ++j) v[j] = m_tanh(v[j]);          // (unrolled: v lives in registers, its indices are compile-time)
  }
}

template <typename T> MDS_HD void policy_features(V3<T> p, V3<T> target, V3<T> rpy, V3<T> v, V3<T> av, T x[kPolicyIn]) {
  const V3<T> e = p - target;
  x[0] = e.x; x[1] = e.y; x[2] = e.z;
  x[3] = rpy.x; x[4] = rpy.y; x[5] = rpy.z;
  x[6] = v.x; x[7] = v.y; x[8] = v.z;
  x[9] = av.x; x[10] = av.y; x[11] = av.z;
}
// the same from an observation row o[20] and the drone's world-frame target
template <typename T> MDS_HD void policy_features_obs(const T o[20], V3<T> target_world, T x[kPolicyIn]) {
  policy_features(V3<T>{o[0], o[1], o[2]}, target_world, V3<T>{o[7], o[8], o[9]}, V3<T>{o[10], o[11], o[12]}, V3<T>{o[13], o[14], o[15]}, x);
}

// y[4] = the network's output for the features x, any width in 1..64: the definition.  WP: a pointer to the packed weights in T.
template <typename T, typename WP> MDS_HD void policy_eval(WP w, int n_hidden, int width, int activation, const T x[kPolicyIn], T y[kPolicyOut]) {
  T a[kPolicyMaxWidth], b[kPolicyMaxWidth];
  for (int j = 0; j < width; ++j) {
    T acc = w[kPolicyIn * width + j];
    for (int k = 0; k < kPolicyIn; ++k) acc = m_fma((T)w[j * kPolicyIn + k], x[k], acc);
    a[j] = policy_act(activation, acc);
  }
  w += (kPolicyIn + 1) * width;
  if (n_hidden == 2) {
    for (int j = 0; j < width; ++j) {
      T acc = w[width * width + j];
      for (int k = 0; k < width; ++k) acc = m_fma((T)w[j * width + k], a[k], acc);
      b[j] = policy_act(activation, acc);
    }
    for (int j = 0; j < width; ++j) a[j] = b[j];
    w += (width + 1) * width;
  }
  for (int o = 0; o < kPolicyOut; ++o) {
    T acc = w[kPolicyOut * width + o];
    for (int k = 0; k < width; ++k) acc = m_fma((T)w[o * width + k], a[k], acc);
    y[o] = acc;
  }
}

// The fixed-width form (the kernels': W one of kPolicyWidths, the weights padded to it): the same chains, arranged for a lane that
// keeps its activations in registers and takes every weight as a wave-uniform operand.  The first hidden layer is held (h[W],
// compile-time indices only); the second never is: as neuron j of layer 2 is finished, W3[o][j] act(h2_j) goes into the four output
// accumulators -- j ascending, the output's own chain.  Four neurons' chains run side by side (one chain alone is W dependent FMAs).
//
// The weights are fetched in chunks, one chunk ahead of the FMAs that use it, and the chunks are fenced off from each other: on the
// device a weight occupies scalar registers from its load to its FMA, and an unfenced block of several hundred FMAs lets the
// scheduler start far more loads than there are scalar registers to hold them.  So that a chunk is one contiguous run of memory
// whatever the number of chains it feeds, the fixed-width form reads the DEVICE LAYOUT (policy_device_layout, applied on upload after
// the padding): every block evaluated four chains at a time -- layer 2 in groups of four neurons, and the output layer of a
// one-hidden-layer policy -- has its four rows interleaved k-major, [k][4]; everything else stays as torch packs it.
#if defined(__HIP_DEVICE_COMPILE__)
#define MDS_POLICY_FENCE() __builtin_amdgcn_sched_barrier(0)
#else
#define MDS_POLICY_FENCE() ((void)0)
#endif
constexpr int kPolicyLanes = 4;
// src: a policy of width W as torch packs it -> dst: the device layout (the same number of weights)
template <typename A, typename B> inline void policy_device_layout(const A* src, int n_hidden, int W, B* dst) {
  const int n1 = (kPolicyIn + 1) * W;
  for (int k = 0; k < n1; ++k) dst[k] = (B)src[k];
  src += n1;
  dst += n1;
  if (n_hidden == 2) {
    for (int j0 = 0; j0 < W; j0 += kPolicyLanes)
      for (int k = 0; k < W; ++k)
        for (int jj = 0; jj < kPolicyLanes; ++jj) dst[j0 * W + k * kPolicyLanes + jj] = (B)src[(j0 + jj) * W + k];
    for (int k = W * W; k < (W + 1) * W + (W + 1) * kPolicyOut; ++k) dst[k] = (B)src[k];        // b2, W3 row-major, b3
  } else {
    for (int k = 0; k < W; ++k)
      for (int o = 0; o < kPolicyOut; ++o) dst[k * kPolicyOut + o] = (B)src[o * W + k];
    for (int o = 0; o < kPolicyOut; ++o) dst[kPolicyOut * W + o] = (B)src[kPolicyOut * W + o];
  }
}
template <int N, typename T, typename WP> MDS_HD void policy_fetch(WP w, T* out) {
#if defined(__clang__)
#pragma unroll
#endif
  for (int k = 0; k < N; ++k) out[k] = (T)w[k];
}
// acc[jj] = bias[jj] + the chain over k = 0 .. W-1 of rows[k * 4 + jj] h[k], jj = 0 .. 3 (rows: four rows interleaved k-major).
// A chunk is 64 bytes, one scalar load of 16 words: 4 (float) or 2 (double) steps of the four chains.  (128-byte chunks, two in
// flight, already made the register allocator spill scalar registers in the small stand-alone kernel.)
template <typename T, int W, typename WP> MDS_HD void policy_dot4(WP rows, WP bias, const T* h, T acc[kPolicyLanes]) {
  constexpr int KC = 16 / (int)sizeof(T), NK = W / KC, CE = KC * kPolicyLanes;
  static_assert(W % KC == 0, "width");
  T wa[CE], wb[CE];
  policy_fetch<kPolicyLanes>(bias, acc);
  policy_fetch<CE>(rows, wa);
#if defined(__clang__)
#pragma unroll
#endif
  for (int kc = 0; kc < NK; ++kc) {
    if (kc + 1 < NK) policy_fetch<CE>(rows + (kc + 1) * CE, wb);
#if defined(__clang__)
#pragma unroll
#endif
    for (int k = 0; k < KC; ++k)
      for (int jj = 0; jj < kPolicyLanes; ++jj) acc[jj] = m_fma(wa[k * kPolicyLanes + jj], h[kc * KC + k], acc[jj]);
    MDS_POLICY_FENCE();
    if (kc + 1 < NK)
      for (int k = 0; k < CE; ++k) wa[k] = wb[k];
  }
}
template <typename T, int W, typename WP> MDS_HD void policy_eval_w(WP w, int n_hidden, int activation, const T x[kPolicyIn], T y[kPolicyOut]) {
  static_assert(W % kPolicyLanes == 0 && W <= kPolicyMaxWidth, "width");
  constexpr int G1 = 8 / (int)sizeof(T), NG = W / G1;          // layer 1: G1 neurons (rows of 12 weights) per group
  T h[W];
  {
    T wa[G1 * kPolicyIn], wb[G1 * kPolicyIn], ba[G1], bb[G1];
    policy_fetch<G1 * kPolicyIn>(w, wa);
    policy_fetch<G1>(w + kPolicyIn * W, ba);
#if defined(__clang__)
#pragma unroll
#endif
    for (int g = 0; g < NG; ++g) {
      if (g + 1 < NG) {
        policy_fetch<G1 * kPolicyIn>(w + (g + 1) * G1 * kPolicyIn, wb);
        policy_fetch<G1>(w + kPolicyIn * W + (g + 1) * G1, bb);
      }
      for (int jj = 0; jj < G1; ++jj) {
        T acc = ba[jj];
#if defined(__clang__)
#pragma unroll
#endif
        for (int k = 0; k < kPolicyIn; ++k) acc = m_fma(wa[jj * kPolicyIn + k], x[k], acc);
        h[g * G1 + jj] = acc;
      }
      MDS_POLICY_FENCE();
      if (g + 1 < NG) {
        for (int k = 0; k < G1 * kPolicyIn; ++k) wa[k] = wb[k];
        for (int k = 0; k < G1; ++k) ba[k] = bb[k];
      }
    }
  }
  policy_act_n<W>(activation, h);
  w += (kPolicyIn + 1) * W;
  if (n_hidden == 2) {
    WP w3 = w + (W + 1) * W;
    policy_fetch<kPolicyOut>(w3 + kPolicyOut * W, y);
#if defined(__clang__)
#pragma unroll 1
#endif
    for (int j0 = 0; j0 < W; j0 += kPolicyLanes) {             // (a loop at run time: its body is the unit the instruction cache holds)
      T acc[kPolicyLanes], wo[kPolicyOut * kPolicyLanes];
      for (int o = 0; o < kPolicyOut; ++o) policy_fetch<kPolicyLanes>(w3 + o * W + j0, wo + o * kPolicyLanes);
      policy_dot4<T, W>(w + j0 * W, w + W * W + j0, h, acc);
      policy_act_n<kPolicyLanes>(activation, acc);
      for (int jj = 0; jj < kPolicyLanes; ++jj)
        for (int o = 0; o < kPolicyOut; ++o) y[o] = m_fma(wo[o * kPolicyLanes + jj], acc[jj], y[o]);
      MDS_POLICY_FENCE();
    }
  } else {
    policy_dot4<T, W>(w, w + kPolicyOut * W, h, y);
  }
}

// the commanded RPM of the network's output
template <typename T> MDS_HD void policy_rpm(const T y[kPolicyOut], T rpm_base, T rpm_scale, T rpm[kPolicyOut]) {
  for (int j = 0; j < kPolicyOut; ++j) rpm[j] = m_fma(rpm_scale, m_clamp(y[j], T(-1), T(1)), rpm_base);
}

}  // namespace mds
