// The continuous algebraic Riccati equation  A^T P + P A - P G P + Q = 0,  G = B R^-1 B^T,  of the dLQR gains
// (DecentralizedLQR / DecentralizedLQROmega.compute_controller), float64 only, as templates on the number of states NS and inputs NU
// of one problem (one drone: 12 / 4 or 9 / 4; the coupled pair of the 12-state model: 24 / 8).  Host-compilable like
// mds_fedce_omega.hpp; the device kernels (mds_care_kernels.hip) run the same functions with one wavefront per problem.
//
//   care_gj_inverse : in-place Gauss-Jordan inverse with partial pivoting; log |det| is the sum of the pivots' logarithms.
//   care_solve      : the matrix sign function of the Hamiltonian Z0 = [[A, -G], [-Q, -A^T]] by the scaled Newton iteration
//                     Z <- (c Z + (c Z)^-1) / 2, c = |det Z|^(-1/2n) (Byers 1987; Higham, "Functions of Matrices", ch. 5), stopped at
//                     |Znew - Z|_1 <= 1e-14 |Znew|_1; with W = sign(Z0) in n x n blocks P = -W21 (I - W11)^-1, symmetrised; then
//                     the relative residual |A^T P + P A - P G P + Q|_1 / |Q|_1 = |[P, -I] Z0 [I; P]|_1 / |Q|_1.
//   care_gain       : K = R^-1 B^T P.
//
// The work is written per COLUMN: x.cols(n, f) runs f(c) for every column c < n and is a barrier; between two barriers a column
// reads what earlier phases wrote and writes only its own entries (or, where said, its own row).  CareSerial runs the columns in
// turn on one thread; the kernels' policy gives column c to lane c.  Data-dependent row indices (the pivot row, the row permutation)
// are read from the work arrays, never from a register array.
#pragma once
#include "mds_math.hpp"

namespace mds {

// status bits of a problem (0: solved); any bit set means no gain is produced
constexpr int kCareCap = 1;          // the iteration cap was reached before the stopping test held
constexpr int kCareSingular = 2;     // a zero or non-finite pivot, or a non-finite result
constexpr int kCareResidual = 4;     // the relative residual is above kCareResidualTol
constexpr int kCareMaxIter = 32;     // default cap (the hover models take 8 to 10 iterations)
constexpr double kCareStop = 1e-14;  // |Znew - Z|_1 <= kCareStop |Znew|_1
// one order of magnitude over the worst residual measured on the reference's own models and on 600 perturbed hover models
// (7.9e-13; tests/test_care_cpu.py prints them)
constexpr double kCareResidualTol = 1e-11;

template <typename T> MDS_HD bool care_finite(T x) { return (x - x) == T(0); }       // false for NaN and +-inf

// Work arrays of one problem: two (2 NS) x (2 NS) matrices with the row stride LD = 2 NS + 1 (odd: a column walk touches every LDS
// bank once), the multiplier column and the pivot rows.
template <int NS> struct CareWork {
  static constexpr int N = 2 * NS, LD = N + 1;
  double Z[N * LD], W[N * LD], mcol[N];
  int piv[N];
};

struct CareSerial {
  template <typename F> MDS_HD void cols(int n, const F& f) const {
    for (int c = 0; c < n; ++c) f(c);
  }
  template <typename F> MDS_HD double sum(int n, const F& f) const {
    double s = 0.0;
    for (int c = 0; c < n; ++c) s += f(c);
    return s;
  }
  template <typename F> MDS_HD double max(int n, const F& f) const {          // of non-negative values; a NaN is returned as one
    double m = 0.0;
    for (int c = 0; c < n; ++c) {
      const double v = f(c);
      m = (v > m || v != v) ? v : m;
    }
    return m;
  }
  // the first c in [lo, n) with the largest f(c)
  template <typename F> MDS_HD int argmax(int lo, int n, const F& f) const {
    int best = lo;
    double bv = f(lo);
    for (int c = lo + 1; c < n; ++c) {
      const double v = f(c);
      if (v > bv) { bv = v; best = c; }
    }
    return best;
  }
};

// a[0:n, 0:n] (row stride LD) <- its inverse.  Returns false at a zero or non-finite pivot (a is then garbage).
template <int LD, typename X> MDS_HD bool care_gj_inverse(const X& x, double* a, int n, double* mcol, int* piv, double* log_abs_det) {
  double lad = 0.0;
  for (int p = 0; p < n; ++p) {
    x.cols(n, [&](int i) { mcol[i] = a[i * LD + p]; });
    const int r = x.argmax(p, n, [&](int i) { return m_abs(mcol[i]); });
    const double d = mcol[r];
    if (!(m_abs(d) > 0.0) || !care_finite(d)) return false;
    lad += log(m_abs(d));
    x.cols(1, [&](int) {
      piv[p] = r;
      mcol[r] = mcol[p];           // row r now holds what row p held; row p is not eliminated
    });
    x.cols(n, [&](int c) {
      const double t = a[r * LD + c];
      if (r != p) a[r * LD + c] = a[p * LD + c];
      const double pr = (c == p ? 1.0 : t) / d;
      a[p * LD + c] = pr;
      for (int i = 0; i < n; ++i) {
        if (i == p) continue;
        const double old = c == p ? 0.0 : a[i * LD + c];
        a[i * LD + c] = m_fma(-mcol[i], pr, old);
      }
    });
  }
  for (int p = n - 1; p >= 0; --p) {       // the row swaps of the elimination are column swaps of the inverse, undone last first
    const int r = piv[p];
    if (r != p)
      x.cols(n, [&](int i) {                // (row i here)
        const double t = a[i * LD + p];
        a[i * LD + p] = a[i * LD + r];
        a[i * LD + r] = t;
      });
  }
  *log_abs_det = lad;
  return true;
}

// Z <- [[A, -G], [-Q, -A^T]] from A [NS, NS], B [NS, NU], R^-1 [NU, NU] and Q [NS, NS] (row-major)
template <int NS, int NU, typename X>
MDS_HD void care_hamiltonian(const X& x, const double* A, const double* B, const double* Rinv, const double* Q, double* Z) {
  constexpr int N = 2 * NS, LD = N + 1;
  x.cols(N, [&](int c) {
    if (c < NS) {
      for (int i = 0; i < NS; ++i) {
        Z[i * LD + c] = A[i * NS + c];
        Z[(NS + i) * LD + c] = -Q[i * NS + c];
      }
    } else {
      const int j = c - NS;
      double v[NU];                       // R^-1 B^T e_j
      for (int q = 0; q < NU; ++q) {
        double s = 0.0;
        for (int r = 0; r < NU; ++r) s = m_fma(Rinv[q * NU + r], B[j * NU + r], s);
        v[q] = s;
      }
      for (int i = 0; i < NS; ++i) {
        double g = 0.0;
        for (int q = 0; q < NU; ++q) g = m_fma(B[i * NU + q], v[q], g);
        Z[i * LD + c] = -g;
        Z[(NS + i) * LD + c] = -A[j * NS + i];
      }
    }
  });
}

// The stabilising solution of the Riccati equation of (A, B, R^-1, Q).  Returns the status bits; with 0, P [NS, NS] is
// w.W[(NS + i) * LD + j].  *iters = Newton iterations taken, *residual = the relative residual (NaN where it was not reached).
template <int NS, int NU, typename X>
MDS_HD int care_solve(const X& x, const double* A, const double* B, const double* Rinv, const double* Q, CareWork<NS>& w, int max_iter,
                      int* iters, double* residual) {
  constexpr int N = 2 * NS, LD = N + 1;
  double* Z = w.Z;
  double* W = w.W;
  *iters = 0;
  *residual = NAN;
  care_hamiltonian<NS, NU>(x, A, B, Rinv, Q, Z);
  bool done = false;
  int it = 0;
  while (it < max_iter && !done) {
    ++it;
    x.cols(N, [&](int c) {
      for (int i = 0; i < N; ++i) W[i * LD + c] = Z[i * LD + c];
    });
    double lad;
    if (!care_gj_inverse<LD>(x, W, N, w.mcol, w.piv, &lad)) {
      *iters = it;
      return kCareSingular;
    }
    const double cs = exp(-lad / N), ci = 1.0 / cs;
    // column c's |Znew - Z| and |Znew| sums are parked in mcol[c] and W[c] (row 0 of W is read before it is overwritten)
    x.cols(N, [&](int c) {
      double dn = 0.0, zn = 0.0;
      for (int i = 0; i < N; ++i) {
        const double z = Z[i * LD + c];
        const double zn1 = 0.5 * m_fma(cs, z, ci * W[i * LD + c]);
        dn += m_abs(zn1 - z);
        zn += m_abs(zn1);
        Z[i * LD + c] = zn1;
      }
      w.mcol[c] = dn;
      W[c] = zn;
    });
    const double dn = x.max(N, [&](int c) { return w.mcol[c]; });
    const double zn = x.max(N, [&](int c) { return W[c]; });
    if (!care_finite(dn) || !care_finite(zn)) {
      *iters = it;
      return kCareSingular;
    }
    done = dn <= kCareStop * zn;
  }
  *iters = it;
  if (!done) return kCareCap;
  // P~ = -W21 (I - W11)^-1 into W's upper right block
  x.cols(NS, [&](int c) {
    for (int i = 0; i < NS; ++i) W[i * LD + c] = (i == c ? 1.0 : 0.0) - Z[i * LD + c];
  });
  double lad;
  if (!care_gj_inverse<LD>(x, W, NS, w.mcol, w.piv, &lad)) return kCareSingular;
  x.cols(NS, [&](int c) {
    for (int i = 0; i < NS; ++i) {
      double s = 0.0;
      for (int k = 0; k < NS; ++k) s = m_fma(Z[(NS + i) * LD + k], W[k * LD + c], s);
      W[i * LD + NS + c] = -s;
    }
  });
  // P = (P~ + P~^T) / 2 into W's lower left block
  x.cols(NS, [&](int c) {
    for (int i = 0; i < NS; ++i) W[(NS + i) * LD + c] = 0.5 * (W[i * LD + NS + c] + W[c * LD + NS + i]);
  });
  // T = Z0 [I; P] [N, NS] into W's right half, then the columns of P T[0:NS] - T[NS:N]
  care_hamiltonian<NS, NU>(x, A, B, Rinv, Q, Z);
  x.cols(NS, [&](int c) {
    for (int k = 0; k < N; ++k) {
      double s = Z[k * LD + c];
      for (int i = 0; i < NS; ++i) s = m_fma(Z[k * LD + NS + i], W[(NS + i) * LD + c], s);
      W[k * LD + NS + c] = s;
    }
  });
  x.cols(NS, [&](int c) {
    double rn = 0.0, qn = 0.0, pn = 0.0;
    for (int i = 0; i < NS; ++i) {
      double s = -W[(NS + i) * LD + NS + c];
      for (int k = 0; k < NS; ++k) s = m_fma(W[(NS + i) * LD + k], W[k * LD + NS + c], s);
      rn += m_abs(s);
      qn += m_abs(Z[(NS + i) * LD + c]);
      pn += m_abs(W[(NS + i) * LD + c]);
    }
    w.mcol[c] = rn;
    w.mcol[NS + c] = qn;
    Z[c] = pn;
  });
  const double rn = x.max(NS, [&](int c) { return w.mcol[c]; });
  const double qn = x.max(NS, [&](int c) { return w.mcol[NS + c]; });
  const double pn = x.max(NS, [&](int c) { return Z[c]; });
  const double res = rn / qn;
  *residual = res;
  if (!care_finite(res) || !care_finite(pn)) return kCareSingular;
  return res > kCareResidualTol ? kCareResidual : 0;
}

// K = R^-1 B^T P [NU, NS], P from care_solve's work arrays; put(q, j, K[q][j]) is called once per entry, column j by column j
template <int NS, int NU, typename X, typename PUT>
MDS_HD void care_gain(const X& x, const double* B, const double* Rinv, const CareWork<NS>& w, const PUT& put) {
  constexpr int LD = 2 * NS + 1;
  x.cols(NS, [&](int c) {
    double t[NU];                         // B^T P e_c
    for (int r = 0; r < NU; ++r) {
      double s = 0.0;
      for (int i = 0; i < NS; ++i) s = m_fma(B[i * NU + r], w.W[(NS + i) * LD + c], s);
      t[r] = s;
    }
    for (int q = 0; q < NU; ++q) {
      double s = 0.0;
      for (int r = 0; r < NU; ++r) s = m_fma(Rinv[q * NU + r], t[r], s);
      put(q, c, s);
    }
  });
}

// A [M, M] and B [M, 4] (row-major) of one drone from its learner state
// 12-state: the 12 free entries f of theta (mds_fedce_kernels.hip: A[6,1], A[7,0], B[3:6,1:4], B[8,0]; A[0:3,3:6] = A[9:12,6:9] = I)
MDS_HD double care_model12_A(const double* f, int i, int j) {
  if (i < 3 && j == i + 3) return 1.0;
  if (i >= 9 && j == i - 3) return 1.0;
  if (i == 6 && j == 1) return f[0];
  if (i == 7 && j == 0) return f[1];
  return 0.0;
}
MDS_HD double care_model12_B(const double* f, int i, int q) {
  if (i >= 3 && i < 6 && q >= 1) return f[2 + 3 * (i - 3) + (q - 1)];
  if (i == 8 && q == 0) return f[11];
  return 0.0;
}
// 9-state: the full theta = [A^T; B^T] [13, 9]
MDS_HD double care_model9_A(const double* th, int i, int j) { return th[j * 9 + i]; }
MDS_HD double care_model9_B(const double* th, int i, int q) { return th[(9 + q) * 9 + i]; }

}  // namespace mds
