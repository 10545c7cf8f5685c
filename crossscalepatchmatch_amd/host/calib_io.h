// calib_io.h -- reader for the calib.txt of the Middlebury 2014 stereo datasets, the calibration cspm_reproject takes (include/cspm.h
// "reprojection").  The file is lines of key=value:
//     cam0=[f 0 cx; 0 f cy; 0 0 1]   cam1=[f 0 cx1; 0 f cy; 0 0 1]   doffs=   baseline=   width=   height=   (ndisp, isint, vmin, vmax, ...)
// cam0, cam1, doffs, baseline, width and height are read, every other key is ignored.  Anything malformed (a key missing, a value that
// is not a number, a truncated matrix, an empty file) returns false: the reader never throws and never reads past the buffer.
#pragma once
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/cspm.h"

struct CalibFile {
  cspm_calib calib;  // f, cx, cy of cam0; baseline; doffs
  double cx1;        // cam1's principal point (doffs = cx1 - cx0 in the dataset's files)
  int width, height; // the image size the numbers belong to
};

namespace calib_io_detail {
// a number at text[pos ..), which must end at a delimiter; advances pos.  strtod needs a terminated string: the token is copied out.
inline bool Number(const std::string &text, size_t *pos, double *out) {
  size_t p = *pos;
  while (p < text.size() && (text[p] == ' ' || text[p] == '\t')) ++p;
  size_t e = p;
  while (e < text.size() && std::strchr("+-.0123456789eE", text[e]) != nullptr && text[e] != '\0') ++e;
  if (e == p || e - p > 63) return false;
  char buf[64];
  std::memcpy(buf, text.data() + p, e - p);
  buf[e - p] = '\0';
  char *end = nullptr;
  const double v = std::strtod(buf, &end);
  if (end != buf + (e - p) || !std::isfinite(v)) return false;
  *out = v;
  *pos = e;
  return true;
}
inline bool Skip(const std::string &text, size_t *pos, char c) {
  size_t p = *pos;
  while (p < text.size() && (text[p] == ' ' || text[p] == '\t')) ++p;
  if (p >= text.size() || text[p] != c) return false;
  *pos = p + 1;
  return true;
}
// [a b c; d e f; g h i] -> nine numbers
inline bool Matrix(const std::string &v, double m[9]) {
  size_t p = 0;
  if (!Skip(v, &p, '[')) return false;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c)
      if (!Number(v, &p, &m[3 * r + c])) return false;
    if (!Skip(v, &p, r < 2 ? ';' : ']')) return false;
  }
  while (p < v.size() && (v[p] == ' ' || v[p] == '\t' || v[p] == '\r')) ++p;
  return p == v.size();
}
inline bool Scalar(const std::string &v, double *out) {
  size_t p = 0;
  if (!Number(v, &p, out)) return false;
  while (p < v.size() && (v[p] == ' ' || v[p] == '\t' || v[p] == '\r')) ++p;
  return p == v.size();
}
}  // namespace calib_io_detail

// the text of a calib.txt (size bytes, not necessarily terminated)
inline bool ParseCalib(const char *text, size_t size, CalibFile *out) {
  if (!text || !out) return false;
  const std::string all(text, size);
  double cam0[9], cam1[9], doffs = 0, baseline = 0, width = 0, height = 0;
  unsigned seen = 0;
  size_t pos = 0;
  while (pos < all.size()) {
    size_t eol = all.find('\n', pos);
    if (eol == std::string::npos) eol = all.size();
    const std::string line = all.substr(pos, eol - pos);
    pos = eol + 1;
    const size_t eq = line.find('=');
    if (eq == std::string::npos) {
      if (line.find_first_not_of(" \t\r") != std::string::npos) return false;  // a line that is no key=value
      continue;
    }
    const std::string key = line.substr(0, eq), val = line.substr(eq + 1);
    using namespace calib_io_detail;
    if (key == "cam0") { if (!Matrix(val, cam0)) return false; seen |= 1u; }
    else if (key == "cam1") { if (!Matrix(val, cam1)) return false; seen |= 2u; }
    else if (key == "doffs") { if (!Scalar(val, &doffs)) return false; seen |= 4u; }
    else if (key == "baseline") { if (!Scalar(val, &baseline)) return false; seen |= 8u; }
    else if (key == "width") { if (!Scalar(val, &width)) return false; seen |= 16u; }
    else if (key == "height") { if (!Scalar(val, &height)) return false; seen |= 32u; }
  }
  if (seen != 63u) return false;
  if (!(cam0[0] > 0.0) || !(baseline > 0.0) || !(width >= 1.0 && width <= 1e6) || !(height >= 1.0 && height <= 1e6)) return false;
  if (width != std::floor(width) || height != std::floor(height)) return false;
  out->calib.f = cam0[0];
  out->calib.cx = cam0[2];
  out->calib.cy = cam0[5];
  out->calib.baseline = baseline;
  out->calib.doffs = doffs;
  out->cx1 = cam1[2];
  out->width = (int)width;
  out->height = (int)height;
  return true;
}

// the calibration of images of width image_w: when the file's width differs (a half- or quarter-size copy of the pair) f, cx, cy and
// doffs are scaled by image_w / width; the baseline is a length and stays
inline cspm_calib ScaledCalib(const CalibFile &c, int image_w) {
  cspm_calib k = c.calib;
  if (image_w != c.width) {
    const double s = (double)image_w / (double)c.width;
    k.f *= s; k.cx *= s; k.cy *= s; k.doffs *= s;
  }
  return k;
}

inline bool ReadCalibFile(const std::string &path, CalibFile *out) {
  FILE *fp = std::fopen(path.c_str(), "rb");
  if (!fp) return false;
  std::string text;
  char buf[4096];
  size_t n;
  while ((n = std::fread(buf, 1, sizeof buf, fp)) > 0 && text.size() < (1u << 20)) text.append(buf, n);
  std::fclose(fp);
  return ParseCalib(text.data(), text.size(), out);
}
