// pose_io.h -- a poses file of the depth-map fusion (include/cspm.h "depth-map fusion", cspm_main --fuse_poses): one view per line, 12
// numbers, the row-major [R | t] of the camera -> world pose (P_world = R P_cam + t) of the pair's RECTIFIED left camera:
//     r00 r01 r02 t0  r10 r11 r12 t1  r20 r21 r22 t2
// Blank lines and lines whose first character that is not a blank is '#' are skipped; a '#' behind the twelfth number starts a comment.
// Whether R is a rotation is the library's check (cspm_fuse_depth_maps), not the reader's.
#pragma once
#include <cmath>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

struct CameraPose {
  double R[9];
  double t[3];
};

// 1: a pose was read; 0: nothing on the line; -1: not a pose (fewer or more than 12 numbers, something that is no number, a value that
// is not finite)
inline int ParsePoseLine(const std::string &line, CameraPose *out) {
  const char *s = line.c_str();
  double v[12];
  int n = 0;
  for (;;) {
    while (*s == ' ' || *s == '\t' || *s == '\r' || *s == ',') ++s;
    if (*s == '\0' || *s == '#') break;
    char *end = NULL;
    const double x = std::strtod(s, &end);
    if (end == s || n == 12 || !std::isfinite(x)) return -1;
    if (*end != '\0' && *end != ' ' && *end != '\t' && *end != '\r' && *end != ',' && *end != '#') return -1;
    v[n++] = x;
    s = end;
  }
  if (n == 0) return 0;
  if (n != 12) return -1;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) out->R[3 * i + j] = v[4 * i + j];
    out->t[i] = v[4 * i + 3];
  }
  return 1;
}

// every pose of the file in order; false when the file cannot be opened or a line is not a pose (*bad_line = its number, 0 = the file)
inline bool ReadPoseFile(const std::string &path, std::vector<CameraPose> *out, int *bad_line) {
  out->clear();
  if (bad_line) *bad_line = 0;
  std::ifstream in(path.c_str());
  if (!in) return false;
  std::string line;
  int line_no = 0;
  while (std::getline(in, line)) {
    ++line_no;
    CameraPose p;
    const int rc = ParsePoseLine(line, &p);
    if (rc < 0) {
      if (bad_line) *bad_line = line_no;
      return false;
    }
    if (rc > 0) out->push_back(p);
  }
  return true;
}
