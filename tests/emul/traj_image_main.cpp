// TEST TOOLING ONLY: the layout cases of tests/test_traj_tables_cpu.py once more as a plain host program (linked with
// tests/emul/traj_emul.cpp and built with -fsanitize=address,undefined by that test): every out-of-range index of the image builder or of
// the evaluators' reads of the image ends the program.  argv[1]: the tables the test wrote --
//   int32 n, total, nt | int32 offsets[n + 1] | int32 compound[n] | double segs[total * MDS_SEG_DIM] | double t[nt] | double origin[3 n]
// Exit status 0 = every check held.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/mds.h"

struct TrajImage;
extern "C" {
TrajImage* traj_image_create(const double* segs, const int32_t* offsets, const int32_t* compound, int n, int32_t total, int* status);
void traj_image_free(TrajImage* im);
int traj_image_nu(const TrajImage* im);
void traj_image_info(const TrajImage* im, int i, int* out);
void traj_image_eval(const TrajImage* im, int mode, int nt, const double* t, const double* origin, double* out);
}

static int bad = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      ++bad;                                                       \
      fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #c); \
    }                                                              \
  } while (0)

static int status_of(const std::vector<double>& segs, const std::vector<int32_t>& off, const std::vector<int32_t>& comp, int32_t total) {
  int st = 0;
  TrajImage* im = traj_image_create(segs.data(), off.data(), comp.data(), (int)comp.size(), total, &st);
  if (im) traj_image_free(im);
  return st;
}

static std::vector<double> wait_rows(int k) {
  std::vector<double> s((size_t)k * MDS_SEG_DIM, 0.0);
  for (int j = 0; j < k; ++j) {
    double* r = s.data() + (size_t)j * MDS_SEG_DIM;
    r[0] = 3.0; r[1] = 0.5 * j; r[2] = 0.5 * (j + 1);
    r[3] = 0.001 * j; r[4] = -1.0; r[5] = 2.0; r[6] = 0.25;
    r[27] = r[31] = r[35] = 1.0;
  }
  return s;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hdr[3];
  if (fread(hdr, 4, 3, f) != 3) return 2;
  const int n = hdr[0], total = hdr[1], nt = hdr[2];
  std::vector<int32_t> off(n + 1), comp(n);
  std::vector<double> segs((size_t)total * MDS_SEG_DIM), t(nt), org((size_t)3 * n);
  if (fread(off.data(), 4, off.size(), f) != off.size() || fread(comp.data(), 4, comp.size(), f) != comp.size() ||
      fread(segs.data(), 8, segs.size(), f) != segs.size() || fread(t.data(), 8, t.size(), f) != t.size() ||
      fread(org.data(), 8, org.size(), f) != org.size())
    return 2;
  fclose(f);

  // the whole set through the builder; every drone equals itself evaluated from a one-table image of its own rows, to the bit
  int st = 0;
  TrajImage* im = traj_image_create(segs.data(), off.data(), comp.data(), n, total, &st);
  CHECK(st == MDS_OK && im);
  if (!im) return 1;
  std::vector<double> all((size_t)nt * n * 11), one((size_t)nt * 11);
  for (int mode = 0; mode < 3; ++mode) {
    traj_image_eval(im, mode, nt, t.data(), org.data(), all.data());
    for (int i = 0; i < n; ++i) {
      const int32_t o1[2] = {0, off[i + 1] - off[i]};
      TrajImage* own = traj_image_create(segs.data() + (size_t)off[i] * MDS_SEG_DIM, o1, &comp[i], 1, o1[1], &st);
      CHECK(st == MDS_OK && own);
      if (!own) return 1;
      traj_image_eval(own, mode, nt, t.data(), org.data() + 3 * i, one.data());
      traj_image_free(own);
      int diff = 0;
      for (int j = 0; j < nt; ++j) diff += memcmp(&all[((size_t)j * n + i) * 11], &one[(size_t)j * 11], 11 * sizeof(double)) != 0;
      if (diff) {
        ++bad;
        fprintf(stderr, "mode %d drone %d: %d of %d times differ from its own one-table image\n", mode, i, diff, nt);
      }
    }
  }
  traj_image_free(im);

  // refusals
  {
    std::vector<double> s = wait_rows(4);
    CHECK(status_of(s, {0, 1, 4}, {0, 1}, 4) == MDS_OK);
    CHECK(status_of(s, {1, 2, 4}, {0, 1}, 4) == MDS_EINVAL);      // offsets[0] != 0
    CHECK(status_of(s, {0, 1, 3}, {0, 1}, 4) == MDS_EINVAL);      // offsets[n] != total
    CHECK(status_of(s, {0, 0, 4}, {0, 1}, 4) == MDS_EINVAL);      // a drone with no piece
    s[0] = -1.0;
    CHECK(status_of(s, {0, 1, 4}, {0, 1}, 4) == MDS_EINVAL);      // kind -1
    s[0] = 3.0;
    s[3 * MDS_SEG_DIM] = 4.0;
    CHECK(status_of(s, {0, 1, 4}, {0, 1}, 4) == MDS_EINVAL);      // kind 4
  }
  // the piece-count limit: 65536 refused, 65535 accepted with the compound bit intact and the last piece reachable
  {
    std::vector<double> s = wait_rows(65536 + 1);
    CHECK(status_of(s, {0, 65536, 65537}, {1, 0}, 65537) == MDS_EINVAL);
    const int32_t o2[3] = {0, 65535, 65536}, c2[2] = {1, 0};
    TrajImage* big = traj_image_create(s.data(), o2, c2, 2, 65536, &st);
    CHECK(st == MDS_OK && big);
    if (big) {
      int info[4];
      traj_image_info(big, 0, info);
      CHECK(info[1] == 65535 && info[2] == 1 && info[3] == 1);
      traj_image_info(big, 1, info);
      CHECK(info[1] == 1 && info[2] == 0);
      const double tt[3] = {0.25, 0.5 * 65534 + 0.25, 1e6}, o0[6] = {0, 0, 0, 0, 0, 0};
      double out[3 * 2 * 11];
      traj_image_eval(big, 0, 3, tt, o0, out);
      CHECK(out[0] == 0.0 && out[2 * 11] == 0.001 * 65534 && out[4 * 11] == 0.001 * 65534);
      traj_image_eval(big, 1, 3, tt, o0, out);
      CHECK(out[0] == 0.0 && out[2 * 11] == (double)(float)(0.001 * 65534));
      traj_image_free(big);
    }
  }
  if (bad) fprintf(stderr, "%d checks failed\n", bad);
  return bad ? 1 : 0;
}
