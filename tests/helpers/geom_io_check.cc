// geom_io_check.cc -- the host layer's calibration reader (host/calib_io.h) and PLY writer (host/ply_io.h), stand-alone: no device, no
// library.  Parses good, scaled and malformed calibration texts and writes the PLY that tests/test_geom_ref.py reads back byte for byte.
// usage: geom_io_check OUT.ply        prints "geom_io_check ok" and exits 0, or says what failed and exits 1
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "calib_io.h"
#include "ply_io.h"

static int g_bad = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);       \
      ++g_bad;                                                    \
    }                                                             \
  } while (0)

// a parse of exactly `s`'s bytes from a heap buffer of exactly that size, so that a read past the end is a sanitizer finding
static bool Parse(const std::string &s, CalibFile *out) {
  std::vector<char> exact(s.begin(), s.end());
  return ParseCalib(exact.empty() ? nullptr : exact.data(), exact.size(), out) ||
         (exact.empty() && ParseCalib("", 0, out));
}

int main(int argc, char **argv) {
  if (argc != 2) {
    std::printf("usage: geom_io_check OUT.ply\n");
    return 2;
  }
  const std::string good =
      "cam0=[3979.911 0 1244.772; 0 3979.911 1019.507; 0 0 1]\n"
      "cam1=[3979.911 0 1369.115; 0 3979.911 1019.507; 0 0 1]\n"
      "doffs=124.343\nbaseline=193.001\nwidth=2964\nheight=2000\nndisp=270\nisint=0\nvmin=23\nvmax=245\ndyavg=0\ndymax=0\n";
  CalibFile c;
  EXPECT(Parse(good, &c));
  EXPECT(c.calib.f == 3979.911 && c.calib.cx == 1244.772 && c.calib.cy == 1019.507 && c.calib.baseline == 193.001 && c.calib.doffs == 124.343);
  EXPECT(c.cx1 == 1369.115 && c.width == 2964 && c.height == 2000);
  // the same size: nothing is scaled; a quarter-size copy: f, cx, cy, doffs times 741 / 2964, the baseline as it is
  cspm_calib k = ScaledCalib(c, 2964);
  EXPECT(k.f == c.calib.f && k.doffs == c.calib.doffs);
  k = ScaledCalib(c, 741);
  const double s = 741.0 / 2964.0;
  EXPECT(k.f == 3979.911 * s && k.cx == 1244.772 * s && k.cy == 1019.507 * s && k.doffs == 124.343 * s && k.baseline == 193.001);
  // CRLF line ends, no final newline, blanks around numbers, keys in another order, exponents
  EXPECT(Parse("width=100\r\nheight=50\r\nbaseline=1e2\r\ndoffs=-2.5\r\ncam1=[ 5e2 0 60 ;0 500 25;0 0 1 ]\r\ncam0=[500 0 50.5; 0 500 25; 0 0 1]", &c));
  EXPECT(c.calib.f == 500.0 && c.calib.cx == 50.5 && c.calib.baseline == 100.0 && c.calib.doffs == -2.5 && c.width == 100 && c.height == 50);

  const char *bad[] = {
      "",                                                                                       // an empty file
      "\n\n",
      "cam0=[1 0 1; 0 1 1; 0 0 1]\n",                                                           // keys missing
      "cam0=[3979.911 0 1244.772; 0 3979.911 1019.507; 0 0 1]\ncam1=[3979.911 0 1369.115; 0 3979.911 1019.507; 0 0 1]\ndoffs=124.343\nbaseline=193.001\nwidth=2964\n",
      "cam0=[3979.911 0 1244.772; 0 3979.911\ncam1=[1 0 1; 0 1 1; 0 0 1]\ndoffs=1\nbaseline=1\nwidth=4\nheight=4\n",  // a truncated matrix
      "cam0=[1 0 1; 0 1 1; 0 0 1\ncam1=[1 0 1; 0 1 1; 0 0 1]\ndoffs=1\nbaseline=1\nwidth=4\nheight=4\n",              // no closing bracket
      "cam0=[1 0 1; 0 1 1; 0 0 1]\ncam1=[1 0 1; 0 1 1; 0 0 1]\ndoffs=abc\nbaseline=1\nwidth=4\nheight=4\n",            // not a number
      "cam0=[1 0 x; 0 1 1; 0 0 1]\ncam1=[1 0 1; 0 1 1; 0 0 1]\ndoffs=1\nbaseline=1\nwidth=4\nheight=4\n",
      "cam0=[1 0 1; 0 1 1; 0 0 1]\ncam1=[1 0 1; 0 1 1; 0 0 1]\ndoffs=1\nbaseline=\nwidth=4\nheight=4\n",               // an empty value
      "cam0=[1 0 1; 0 1 1; 0 0 1]\ncam1=[1 0 1; 0 1 1; 0 0 1]\ndoffs=1 2\nbaseline=1\nwidth=4\nheight=4\n",            // two values
      "cam0=[1 0 1; 0 1 1; 0 0 1]\ncam1=[1 0 1; 0 1 1; 0 0 1]\ndoffs=1\nbaseline=0\nwidth=4\nheight=4\n",              // no baseline
      "cam0=[0 0 1; 0 1 1; 0 0 1]\ncam1=[1 0 1; 0 1 1; 0 0 1]\ndoffs=1\nbaseline=1\nwidth=4\nheight=4\n",              // no focal length
      "cam0=[1 0 1; 0 1 1; 0 0 1]\ncam1=[1 0 1; 0 1 1; 0 0 1]\ndoffs=1\nbaseline=1\nwidth=0\nheight=4\n",
      "cam0=[1 0 1; 0 1 1; 0 0 1]\ncam1=[1 0 1; 0 1 1; 0 0 1]\ndoffs=1e999\nbaseline=1\nwidth=4\nheight=4\n",          // overflows to infinity
      "cam0=[1 0 1; 0 1 1; 0 0 1]\ncam1=[1 0 1; 0 1 1; 0 0 1]\ndoffs=1\nbaseline=1\nwidth=4\nheight=4\nrubbish without a key\n",
      "cam0=[1 0 1; 0 1 1; 0 0 1]\ncam1=[1 0 1; 0 1 1; 0 0 1]\ndoffs=1\nbaseline=1\nwidth=4\nheight",                  // truncated in a key
      "cam0=[1 0 1; 0 1 1; 0 0 1]\ncam1=[1 0 1; 0 1 1; 0 0 1]\ndoffs=1\nbaseline=1\nwidth=4\nheight=1111111111111111111111111111111111111111111111111111111111111111111\n",
  };
  for (size_t i = 0; i < sizeof bad / sizeof bad[0]; ++i) {
    CalibFile t;
    if (Parse(bad[i], &t)) {
      std::printf("FAILED: malformed text %zu was accepted\n", i);
      ++g_bad;
    }
  }
  // every prefix of the good text: no read past the buffer, and none but the whole parses (the last value's digits aside)
  for (size_t n = 0; n < good.size(); ++n) {
    CalibFile t;
    const bool ok = Parse(good.substr(0, n), &t);
    if (ok && n < good.find("vmin")) EXPECT(t.height != 2000 || n >= good.find("height=2000") + 11);
  }
  EXPECT(!ParseCalib(nullptr, 0, &c) && !ParseCalib("x", 1, nullptr));
  EXPECT(!ReadCalibFile(std::string(argv[1]) + ".does-not-exist", &c));

  const float nan = std::numeric_limits<float>::quiet_NaN();
  const cspm_point pts[3] = {{1.f, 2.f, 3.f, 0.f, 0.f, -1.f, 10, 20, 30, 255, 0u},
                             {-0.5f, 0.25f, 8.f, 0.6f, 0.f, -0.8f, 255, 0, 128, 255, 7u},
                             {4.f, 5.f, 6.f, nan, 0.5f, 0.5f, 9, 8, 7, 255, 9u}};
  EXPECT(WritePLY(argv[1], pts, 3));
  EXPECT(!WritePLY(std::string(argv[1]) + ".no-such-dir/x.ply", pts, 3));
  if (g_bad) return 1;
  std::printf("geom_io_check ok\n");
  return 0;
}
