// rig_io.h -- reader for the rig file of cspm_main --rig: the two raw cameras and the pose of camera 1 in camera 0's frame, what
// cspm_rectify_compute takes (include/cspm.h "rectification").  The format is this project's own (INTEGRATION.md "rig files"), lines of
// key=value in any order:
//     cam0=[fx skew cx; 0 fy cy; 0 0 1]     dist0=[k1 k2 p1 p2 k3]
//     cam1=[fx skew cx; 0 fy cy; 0 0 1]     dist1=[k1 k2 p1 p2 k3]
//     R=[r00 r01 r02; r10 r11 r12; r20 r21 r22]     T=[tx ty tz]          X1 = R*X0 + T
//     width=     height=                                                  the size of both raw images
// All eight keys are required, each at most once, every other key is ignored, and so are blank lines and lines that start with '#'.  Anything malformed (a
// key missing or given twice, a value that is not a number, a truncated matrix, a camera matrix whose last two rows are not 0 fy cy; 0 0 1, an empty file)
// returns false: the reader never throws and never reads past the buffer.  Whether the numbers describe a rig that can be rectified is
// cspm_rectify_compute's business.
#pragma once
#include <string>

#include "../../include/cspm.h"
#include "calib_io.h"

namespace rig_io_detail {
// [a b c ...] -> n numbers
inline bool Vector(const std::string &v, int n, double *out) {
  using namespace calib_io_detail;
  size_t p = 0;
  if (!Skip(v, &p, '[')) return false;
  for (int i = 0; i < n; ++i)
    if (!Number(v, &p, &out[i])) return false;
  if (!Skip(v, &p, ']')) return false;
  while (p < v.size() && (v[p] == ' ' || v[p] == '\t' || v[p] == '\r')) ++p;
  return p == v.size();
}
inline bool Camera(const std::string &v, cspm_camera *c) {
  double m[9];
  if (!calib_io_detail::Matrix(v, m)) return false;
  if (m[3] != 0.0 || m[6] != 0.0 || m[7] != 0.0 || m[8] != 1.0) return false;
  c->fx = m[0]; c->skew = m[1]; c->cx = m[2]; c->fy = m[4]; c->cy = m[5];
  return true;
}
inline bool Distortion(const std::string &v, cspm_camera *c) {
  double d[5];
  if (!Vector(v, 5, d)) return false;
  c->k1 = d[0]; c->k2 = d[1]; c->p1 = d[2]; c->p2 = d[3]; c->k3 = d[4];
  return true;
}
}  // namespace rig_io_detail

// the text of a rig file (size bytes, not necessarily terminated)
inline bool ParseRig(const char *text, size_t size, cspm_rig *out) {
  if (!text || !out) return false;
  const std::string all(text, size);
  cspm_rig rig = cspm_rig();
  double width = 0, height = 0;
  unsigned seen = 0;
  size_t pos = 0;
  while (pos < all.size()) {
    size_t eol = all.find('\n', pos);
    if (eol == std::string::npos) eol = all.size();
    const std::string line = all.substr(pos, eol - pos);
    pos = eol + 1;
    const size_t first = line.find_first_not_of(" \t\r");
    if (first == std::string::npos || line[first] == '#') continue;
    const size_t eq = line.find('=');
    if (eq == std::string::npos) return false;  // a line that is no key=value
    const std::string key = line.substr(first, eq - first), val = line.substr(eq + 1);
    using namespace rig_io_detail;
    if (key == "cam0") { if ((seen & 1u) || !Camera(val, &rig.cam[0])) return false; seen |= 1u; }
    else if (key == "dist0") { if ((seen & 2u) || !Distortion(val, &rig.cam[0])) return false; seen |= 2u; }
    else if (key == "cam1") { if ((seen & 4u) || !Camera(val, &rig.cam[1])) return false; seen |= 4u; }
    else if (key == "dist1") { if ((seen & 8u) || !Distortion(val, &rig.cam[1])) return false; seen |= 8u; }
    else if (key == "R") { if ((seen & 16u) || !calib_io_detail::Matrix(val, rig.R)) return false; seen |= 16u; }
    else if (key == "T") { if ((seen & 32u) || !Vector(val, 3, rig.T)) return false; seen |= 32u; }
    else if (key == "width") { if ((seen & 64u) || !calib_io_detail::Scalar(val, &width)) return false; seen |= 64u; }
    else if (key == "height") { if ((seen & 128u) || !calib_io_detail::Scalar(val, &height)) return false; seen |= 128u; }
  }
  if (seen != 255u) return false;
  if (!(width >= 1.0 && width <= 1e6) || !(height >= 1.0 && height <= 1e6) || width != std::floor(width) || height != std::floor(height)) return false;
  rig.raw_w = (int)width;
  rig.raw_h = (int)height;
  *out = rig;
  return true;
}

inline bool ReadRigFile(const std::string &path, cspm_rig *out) {
  FILE *fp = std::fopen(path.c_str(), "rb");
  if (!fp) return false;
  std::string text;
  char buf[4096];
  size_t n;
  while ((n = std::fread(buf, 1, sizeof buf, fp)) > 0 && text.size() < (1u << 20)) text.append(buf, n);
  std::fclose(fp);
  return ParseRig(text.data(), text.size(), out);
}
