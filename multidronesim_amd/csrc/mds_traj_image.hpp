// Host side of the trajectory tables: per-drone segment rows -> the device image that csrc/mds_traj.hpp reads (field-major,
// piece-major blocks, one copy per distinct table) and the 3-int index entry per drone (traj_info).  Pure host code, no HIP:
// mds_set_trajectory_segments uploads what this builds, and the CPU tests build and read the same image (tests/emul/traj_emul.cpp).
#pragma once
#include <stdint.h>
#include <string.h>

#include <new>
#include <unordered_map>
#include <vector>

#include "../../include/mds.h"

namespace mds {

// segs [total, MDS_SEG_DIM] row-major, offsets [n + 1], compound [n] -> fm [MDS_SEG_DIM * nu] (field f of segment id at fm[f * nu + id]),
// tinfo [3 * n] (first, nseg | compound << 16, stride), nu = segments stored.  Returns an mds_status; *why names the refusal.
inline int build_traj_image(const double* segs, const int32_t* offsets, const int32_t* compound, int n, int32_t total,
                            std::vector<double>& fm, std::vector<int>& ti, int& nu, const char** why = nullptr) {
  const char* dummy;
  const char*& msg = why ? *why : dummy;
  msg = "";
  if (total <= 0 || offsets[0] != 0 || offsets[n] != total) return msg = "mds_set_trajectory_segments: offsets", MDS_EINVAL;
  for (int i = 0; i < n; ++i) {
    const int ns = offsets[i + 1] - offsets[i];
    if (ns < 1 || ns > 65535) return msg = "mds_set_trajectory_segments: every drone needs 1..65535 segments", MDS_EINVAL;
  }
  for (int k = 0; k < total; ++k) {
    const int kind = (int)segs[(size_t)k * MDS_SEG_DIM];
    if (kind < 0 || kind > 3) return msg = "mds_set_trajectory_segments: segment kind", MDS_EINVAL;
  }
  // Drones that follow identical tables (the same trajectory objects broadcast over every env) share one device copy:
  // the table then stays in L2 instead of costing up to 300 B of HBM reads per drone-step.  Unique tables with the same
  // number of pieces form a block stored piece-major (TrajInfo), and the image is field-major (SegTable).
  std::vector<int> uniq_of, usrc, uns;     // usrc/uns: first source row / piece count of a unique table
  nu = 0;
  try {
    ti.assign((size_t)3 * n, 0);
    uniq_of.resize((size_t)n);
    std::unordered_multimap<uint64_t, int> seen;        // hash of a drone's rows -> unique table
    for (int i = 0; i < n; ++i) {
      const int ns = offsets[i + 1] - offsets[i];
      const unsigned char* bytes = reinterpret_cast<const unsigned char*>(segs + (size_t)offsets[i] * MDS_SEG_DIM);
      const size_t nbytes = sizeof(double) * MDS_SEG_DIM * (size_t)ns;
      uint64_t hsh = 1469598103934665603ull ^ (uint64_t)ns;
      for (size_t w = 0; w < nbytes; w += 8) {
        uint64_t word;
        memcpy(&word, bytes + w, 8);
        hsh = (hsh ^ word) * 1099511628211ull;
        hsh ^= hsh >> 29;
      }
      int u = -1;
      auto range = seen.equal_range(hsh);
      for (auto it = range.first; it != range.second; ++it) {
        const int j = it->second;
        if (uns[j] == ns && memcmp(bytes, segs + (size_t)usrc[j] * MDS_SEG_DIM, nbytes) == 0) {
          u = j;
          break;
        }
      }
      if (u < 0) {
        u = (int)usrc.size();
        usrc.push_back(offsets[i]);
        uns.push_back(ns);
        seen.emplace(hsh, u);
      }
      uniq_of[i] = u;
    }
    // blocks by piece count, in order of first appearance
    const int nuniq = (int)usrc.size();
    std::unordered_map<int, int> block_of;              // piece count -> block
    std::vector<int> bcount, bns, rank((size_t)nuniq), blk((size_t)nuniq);
    for (int u = 0; u < nuniq; ++u) {
      auto it = block_of.find(uns[u]);
      if (it == block_of.end()) {
        it = block_of.emplace(uns[u], (int)bcount.size()).first;
        bcount.push_back(0);
        bns.push_back(uns[u]);
      }
      blk[u] = it->second;
      rank[u] = bcount[it->second]++;
    }
    std::vector<long long> bbase(bcount.size());
    long long acc = 0;
    for (size_t b = 0; b < bcount.size(); ++b) {
      bbase[b] = acc;
      acc += (long long)bcount[b] * bns[b];
    }
    if (acc > 0x7fffffffll) return msg = "mds_set_trajectory_segments: too many segments", MDS_EINVAL;
    nu = (int)acc;
    fm.assign((size_t)MDS_SEG_DIM * nu, 0.0);
    for (int u = 0; u < nuniq; ++u) {
      const int stride = bcount[blk[u]];
      for (int k = 0; k < uns[u]; ++k) {
        const double* row = segs + (size_t)(usrc[u] + k) * MDS_SEG_DIM;
        const size_t id = (size_t)bbase[blk[u]] + rank[u] + (size_t)k * stride;
        for (int f = 0; f < MDS_SEG_DIM; ++f) fm[(size_t)f * nu + id] = row[f];
        // the affine map is skipped on the device when it is the identity (no RotateTrajectory above this piece)
        bool ident = true;
        for (int r = 0; r < 3; ++r) {
          for (int c = 0; c < 3; ++c) ident = ident && row[27 + 3 * r + c] == (r == c ? 1.0 : 0.0);
          ident = ident && row[36 + r] == 0.0;
        }
        if (!ident) fm[id] = row[0] + 8.0;               // field 0 = kind | kSegAffine
      }
    }
    for (int i = 0; i < n; ++i) {
      const int u = uniq_of[i];
      ti[3 * i] = (int)bbase[blk[u]] + rank[u];
      ti[3 * i + 1] = uns[u] | ((compound[i] ? 1 : 0) << 16);
      ti[3 * i + 2] = bcount[blk[u]];
    }
  } catch (const std::bad_alloc&) {
    return msg = "mds_set_trajectory_segments: host allocation", MDS_ENOMEM;
  }
  return MDS_OK;
}

}  // namespace mds
