// TEST TOOLING ONLY: host build of the two halves of csrc/mds_math.hpp's lemniscate_local and of the periodicity rule of the phase
// table (lemniscate_phase_periodic).  Compiled by tests/test_phase_table_cpu.py with g++: as a shared library for the comparisons from
// NumPy, and as a program of its own (this main) that makes the same two checks on inputs of its own -- the build that runs under
// -fsanitize=address,undefined.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../multidronesim_amd/csrc/mds_math.hpp"

using namespace mds;

// P [7] as uploaded: a, omega, centre3, yaw_rate, phase_shift
template <typename T> static LemniscateParams<T> params_of(const double* p) {
  return LemniscateParams<T>{(T)p[0], (T)p[1], (T)p[2], (T)p[3], (T)p[4], (T)p[5], (T)p[6]};
}
// whole: lemniscate_local(P, t); split: (s, c) = m_sincos(reduced_phase(t, omega, phase_shift)) formed here, as the table's fill
// kernel forms them, then lemniscate_from_sc(P, s, c).  11 values of T each.
template <typename T, bool Y0> static void lem_one(const double* p, double t, T* whole, T* split) {
  static_assert(sizeof(Desired<T>) == 11 * sizeof(T), "Desired is 11 values");
  const LemniscateParams<T> P = params_of<T>(p);
  const Desired<T> w = lemniscate_local<T, Y0>(P, t);
  T s, c;
  m_sincos(reduced_phase<T>(t, P.omega, P.phase_shift), &s, &c);
  const Desired<T> d = lemniscate_from_sc<T, Y0>(P, s, c, t);
  memcpy(whole, &w, sizeof(w));
  memcpy(split, &d, sizeof(d));
}
template <typename T> static void lem_both(int n, const double* P, const double* t, int y0, T* whole, T* split) {
  for (int i = 0; i < n; ++i) {
    if (y0) lem_one<T, true>(P + 7 * i, t[i], whole + 11 * i, split + 11 * i);
    else lem_one<T, false>(P + 7 * i, t[i], whole + 11 * i, split + 11 * i);
  }
}

extern "C" {
void pt_lem_f32(int n, const double* P, const double* t, int y0, float* whole, float* split) { lem_both<float>(n, P, t, y0, whole, split); }
void pt_lem_f64(int n, const double* P, const double* t, int y0, double* whole, double* split) { lem_both<double>(n, P, t, y0, whole, split); }
int pt_phase_periodic(const double* params, long n) { return lemniscate_phase_periodic(params, n) ? 1 : 0; }
}

// ---- the program ----
static unsigned long long g_rng = 0x9e3779b97f4a7c15ull;
static double uni(double lo, double hi) {          // xorshift64*: the inputs need no quality, only spread
  g_rng ^= g_rng >> 12; g_rng ^= g_rng << 25; g_rng ^= g_rng >> 27;
  return lo + (hi - lo) * (double)((g_rng * 0x2545f4914f6cdd1dull) >> 11) / 9007199254740992.0;
}
static double next_up(double x) {
  unsigned long long b;
  memcpy(&b, &x, 8);
  b += x >= 0 ? 1 : -1;
  memcpy(&x, &b, 8);
  return x;
}

template <typename T> static long lem_mismatches(int n) {
  std::vector<double> P((size_t)7 * n), t(n);
  for (int i = 0; i < n; ++i) {
    double* p = &P[(size_t)7 * i];
    p[0] = uni(0.2, 3.0); p[1] = uni(-3.0, 3.0); p[2] = uni(-5, 5); p[3] = uni(-5, 5); p[4] = uni(0, 2);
    p[5] = i % 3 ? uni(-1.0, 1.0) : 0.0; p[6] = uni(-7.0, 7.0);
    t[i] = uni(0.0, 300.0);
  }
  long bad = 0;
  std::vector<T> w((size_t)11 * n), s((size_t)11 * n);
  for (int y0 = 0; y0 < 2; ++y0) {
    lem_both<T>(n, P.data(), t.data(), y0, w.data(), s.data());
    for (size_t k = 0; k < w.size(); ++k) bad += memcmp(&w[k], &s[k], sizeof(T)) != 0;
  }
  return bad;
}

// the rule restated: brute force over every pair of rows 64 apart
static bool periodic_ref(const std::vector<double>& P, long n) {
  bool ok = true;
  for (long i = 0; i + 64 < n; ++i) ok = ok && P[7 * i + 1] == P[7 * (i + 64) + 1] && P[7 * i + 6] == P[7 * (i + 64) + 6];
  return ok;
}
static long periodic_mismatches() {
  long bad = 0;
  const long sizes[] = {1, 63, 64, 65, 128, 259};
  for (long n : sizes) {
    std::vector<double> P((size_t)7 * n);                  // exactly n rows: a read past them is the sanitizer's to report
    for (long i = 0; i < n; ++i) {
      for (int k = 0; k < 7; ++k) P[7 * i + k] = uni(-2, 2);              // the other columns are free
      P[7 * i + 1] = 0.5 + 0.01 * (double)(i % 64);
      P[7 * i + 6] = 0.1 * (double)(i % 64) - 3.0;
    }
    bad += lemniscate_phase_periodic(P.data(), n) != true;
    for (int col : {1, 6})
      for (long row : {64L, n - 1}) {
        if (row < 0 || row >= n) continue;
        std::vector<double> Q = P;
        Q[7 * row + col] = next_up(Q[7 * row + col]);
        const bool want = periodic_ref(Q, n);
        bad += want != (n <= 64);                                          // (a row without a partner 64 away decides nothing)
        bad += lemniscate_phase_periodic(Q.data(), n) != want;
      }
  }
  return bad;
}

int main() {
  const long bad = lem_mismatches<float>(100000) + lem_mismatches<double>(100000);
  const long badp = periodic_mismatches();
  printf("%ld unequal outputs, %ld wrong periodicity decisions\n", bad, badp);
  return bad || badp ? 1 : 0;
}
