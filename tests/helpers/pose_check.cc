// pose_check.cc -- the poses-file reader of the host layer (host/pose_io.h) alone, no library: tests/test_capi_fuse.py runs it plain and
// under AddressSanitizer and UBSan.  pose_check FILE prints "ok N" and the poses, 12 numbers per line in the file's order, or
// "bad LINE" (0 = the file cannot be opened); without an argument it checks single lines and prints "pose_check ok".
#include <cstdio>
#include <cstring>

#include "pose_io.h"

static int fails = 0;
#define CHECK(cond)                                           \
  do {                                                        \
    if (!(cond)) {                                            \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);   \
      ++fails;                                                \
    }                                                         \
  } while (0)

int main(int argc, char **argv) {
  if (argc > 1) {
    std::vector<CameraPose> poses;
    int bad = 0;
    if (!ReadPoseFile(argv[1], &poses, &bad)) {
      std::printf("bad %d\n", bad);
      return 2;
    }
    std::printf("ok %zu\n", poses.size());
    for (size_t k = 0; k < poses.size(); ++k) {
      for (int i = 0; i < 3; ++i) std::printf("%.17g %.17g %.17g %.17g ", poses[k].R[3 * i], poses[k].R[3 * i + 1], poses[k].R[3 * i + 2], poses[k].t[i]);
      std::printf("\n");
    }
    return 0;
  }
  CameraPose p;
  std::memset(&p, 0, sizeof p);
  CHECK(ParsePoseLine("", &p) == 0);
  CHECK(ParsePoseLine("   \t\r", &p) == 0);
  CHECK(ParsePoseLine("# 1 2 3", &p) == 0);
  CHECK(ParsePoseLine("   # indented comment", &p) == 0);
  CHECK(ParsePoseLine("1 2 3 4 5 6 7 8 9 10 11 12", &p) == 1);
  CHECK(p.R[0] == 1 && p.R[1] == 2 && p.R[2] == 3 && p.t[0] == 4 && p.R[3] == 5 && p.R[5] == 7 && p.t[1] == 8 && p.R[6] == 9 && p.R[8] == 11 && p.t[2] == 12);
  CHECK(ParsePoseLine("\t1e0 -2.5 +3 4,5 6 7 8\t9 10 11 1.2e1\r", &p) == 1);
  CHECK(p.R[1] == -2.5 && p.t[2] == 12.0);
  CHECK(ParsePoseLine("1 2 3 4 5 6 7 8 9 10 11 12# tail", &p) == 1);
  CHECK(ParsePoseLine("1 2 3 4 5 6 7 8 9 10 11 12 # tail 13", &p) == 1);
  CHECK(ParsePoseLine("1 2 3 4 5 6 7 8 9 10 11", &p) == -1);
  CHECK(ParsePoseLine("1 2 3 4 5 6 7 8 9 10 11 12 13", &p) == -1);
  CHECK(ParsePoseLine("1 2 3 4 5 6 7 8 9 10 11 x", &p) == -1);
  CHECK(ParsePoseLine("1 2 3 4 5 6 7 8 9 10 11 12x", &p) == -1);
  CHECK(ParsePoseLine("1 2 3 4 5 6 7 8 9 10 11 nan", &p) == -1);
  CHECK(ParsePoseLine("1 2 3 4 5 6 7 8 9 10 inf 12", &p) == -1);
  CHECK(ParsePoseLine("1 2 3 # 4 5 6 7 8 9 10 11 12", &p) == -1);
  if (fails == 0) std::printf("pose_check ok\n");
  return fails ? 1 : 0;
}
