// TEST TOOLING ONLY: host build of the segment-table trajectory path -- the image builder of csrc/mds_traj_image.hpp and the
// evaluators of csrc/mds_traj.hpp (traj_eval, TrajLocal<float>, TrajLocal<double>) reading the image that builder made, exactly as
// the kernels read the uploaded one.  Compiled with g++ by tests/test_traj_tables_cpu.py; tests/emul/traj_image_main.cpp links it.
#include "../../multidronesim_amd/csrc/mds_traj.hpp"
#include "../../multidronesim_amd/csrc/mds_traj_image.hpp"

using namespace mds;

struct TrajImage {
  std::vector<double> fm;
  std::vector<int> tinfo;
  int nu = 0, n = 0;
};

extern "C" {

// -> image (or null), *status = what build_traj_image returned
TrajImage* traj_image_create(const double* segs, const int32_t* offsets, const int32_t* compound, int n, int32_t total, int* status) {
  TrajImage* im = new TrajImage;
  im->n = n;
  *status = build_traj_image(segs, offsets, compound, n, total, im->fm, im->tinfo, im->nu);
  if (*status != MDS_OK) {
    delete im;
    return nullptr;
  }
  return im;
}
void traj_image_free(TrajImage* im) { delete im; }
int traj_image_nu(const TrajImage* im) { return im->nu; }
void traj_image_copy(const TrajImage* im, double* fm, int* tinfo) {
  memcpy(fm, im->fm.data(), sizeof(double) * im->fm.size());
  memcpy(tinfo, im->tinfo.data(), sizeof(int) * im->tinfo.size());
}
// traj_info of drone i -> out[4] = first, nseg, compound, stride
void traj_image_info(const TrajImage* im, int i, int* out) {
  const TrajInfo ti = traj_info(im->tinfo.data(), i);
  out[0] = ti.first; out[1] = ti.nseg; out[2] = ti.compound; out[3] = ti.stride;
}
// every drone at every time -> out [nt, n, 11] (pos3 vel3 acc3 yaw yaw_rate).
//   mode 0: traj_eval (double, world frame)
//   mode 1: TrajLocal<float>::eval with the fp32 origin, returned in the world frame as (double)des.p + (double)(float)origin
//   mode 2: TrajLocal<double>::eval, as returned (relative to origin)
void traj_image_eval(const TrajImage* im, int mode, int nt, const double* t, const double* origin, double* out) {
  const SegTable tb{im->fm.data(), im->nu};
  for (int j = 0; j < nt; ++j)
    for (int i = 0; i < im->n; ++i) {
      double* o = out + ((size_t)j * im->n + i) * 11;
      const TrajInfo ti = traj_info(im->tinfo.data(), i);
      const double* og = origin + 3 * i;
      if (mode == 0) {
        traj_eval(tb, ti, t[j], o);
      } else if (mode == 1) {
        const V3<float> org = {(float)og[0], (float)og[1], (float)og[2]};
        const Desired<float> d = TrajLocal<float>::eval(tb, ti, t[j], org);
        const double v[11] = {(double)d.p.x + (double)org.x, (double)d.p.y + (double)org.y, (double)d.p.z + (double)org.z,
                              d.v.x, d.v.y, d.v.z, d.a.x, d.a.y, d.a.z, d.yaw, d.yaw_rate};
        for (int k = 0; k < 11; ++k) o[k] = v[k];
      } else {
        const V3<double> org = {og[0], og[1], og[2]};
        const Desired<double> d = TrajLocal<double>::eval(tb, ti, t[j], org);
        const double v[11] = {d.p.x, d.p.y, d.p.z, d.v.x, d.v.y, d.v.z, d.a.x, d.a.y, d.a.z, d.yaw, d.yaw_rate};
        for (int k = 0; k < 11; ++k) o[k] = v[k];
      }
    }
}

}  // extern "C"
