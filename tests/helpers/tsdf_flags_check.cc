// tsdf_flags_check.cc -- the flag parsers of the host layer's TSDF volume (host/tsdf_volume.h: ParseTsdfTriple, ParseTsdfDims) alone,
// no library call: tests/test_capi_tsdf.py runs it plain and under AddressSanitizer and UBSan.  tsdf_flags_check triple TEXT prints
// "ok a b c" (%.17g) or "bad"; tsdf_flags_check dims TEXT prints "ok nx ny nz" or "bad"; without an argument it checks a list of texts and
// prints "tsdf_flags_check ok".
#include <cstdio>
#include <cstring>

#include "tsdf_volume.h"

static int fails = 0;
#define CHECK(cond)                                           \
  do {                                                        \
    if (!(cond)) {                                            \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);   \
      ++fails;                                                \
    }                                                         \
  } while (0)

int main(int argc, char **argv) {
  double v[3] = {7.0, 7.0, 7.0};
  int d[3] = {7, 7, 7};
  if (argc > 2 && !std::strcmp(argv[1], "triple")) {
    if (!ParseTsdfTriple(argv[2], v)) return std::printf("bad\n"), 2;
    return std::printf("ok %.17g %.17g %.17g\n", v[0], v[1], v[2]), 0;
  }
  if (argc > 2 && !std::strcmp(argv[1], "dims")) {
    if (!ParseTsdfDims(argv[2], d)) return std::printf("bad\n"), 2;
    return std::printf("ok %d %d %d\n", d[0], d[1], d[2]), 0;
  }
  CHECK(ParseTsdfTriple("1,2,3", v) && v[0] == 1 && v[1] == 2 && v[2] == 3);
  CHECK(ParseTsdfTriple(" -1.5 , 2e-3,\t+0.25", v) && v[0] == -1.5 && v[1] == 2e-3 && v[2] == 0.25);
  CHECK(ParseTsdfTriple("inf,nan,0", v) && v[2] == 0);  // parsed; the range checks refuse them
  CHECK(!ParseTsdfTriple(NULL, v));
  CHECK(!ParseTsdfTriple("", v));
  CHECK(!ParseTsdfTriple("1,2", v));
  CHECK(!ParseTsdfTriple("1,2,", v));
  CHECK(!ParseTsdfTriple("1,2,3,", v));
  CHECK(!ParseTsdfTriple("1,2,3,4", v));
  CHECK(!ParseTsdfTriple("1 2 3", v));
  CHECK(!ParseTsdfTriple("1,,3", v));
  CHECK(!ParseTsdfTriple("1,2,3x", v));
  CHECK(!ParseTsdfTriple(",1,2,3", v));
  CHECK(ParseTsdfDims("96,96,64", d) && d[0] == 96 && d[1] == 96 && d[2] == 64);
  CHECK(ParseTsdfDims("0,-1,2147483647", d) && d[0] == 0 && d[1] == -1 && d[2] == 2147483647);  // the range checks refuse them
  CHECK(!ParseTsdfDims("1.5,2,3", d));
  CHECK(!ParseTsdfDims("1,2,2147483648", d));
  CHECK(!ParseTsdfDims("1,2,1e30", d));
  CHECK(!ParseTsdfDims("1,2,nan", d));
  CHECK(!ParseTsdfDims("1,2,inf", d));
  CHECK(!ParseTsdfDims("1,2", d));
  if (!fails) std::printf("tsdf_flags_check ok\n");
  return fails ? 1 : 0;
}
