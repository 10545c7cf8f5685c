// rect_check.cc -- the host layer's rectification entries against each other and against the C ABI: RectifyPair equals
// cspm_rectify_host per view; a cost object made from the RAW pair through a DeviceSlot with SetRectification works on exactly
// RectifyPair's images (LevelImages) and keeps doing so for a second pair on the parked context; the CSPatchMatch constructor for raw
// pairs gives the maps of the ordinary constructor on the rectified pair; a raw pair of another size throws; the rig reader reads what
// it is documented to read.
// usage: rect_check        prints "rect_check ok" and exits 0, or says what failed and exits 1
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "cs_patchmatch.h"
#include "cc/grd_cc.h"
#include "plane_cost/pre_ss_pc.h"
#include "rig_io.h"

static int g_bad = 0;
#define EXPECT(cond)                                        \
  do {                                                      \
    if (!(cond)) {                                          \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
      ++g_bad;                                              \
    }                                                       \
  } while (0)

static bool SameMat(const Mat &a, const Mat &b) {
  if (a.rows != b.rows || a.cols != b.cols || a.type() != b.type()) return false;
  for (int y = 0; y < a.rows; ++y)
    if (std::memcmp(a.ptr<unsigned char>(y), b.ptr<unsigned char>(y), (size_t)a.cols * a.elemSize()) != 0) return false;
  return true;
}

static Mat Noise(int w, int h, unsigned seed) {
  Mat m(h, w, CV_8UC3);
  unsigned s = seed;
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < 3 * w; ++x) {
      s = s * 1664525u + 1013904223u;
      m.ptr<unsigned char>(y)[x] = (unsigned char)(((x / 3 * 5 + y * 11) & 63) * 3 + ((s >> 24) & 31));
    }
  return m;
}

int main() {
  const char *text =
      "# a small rig\n"
      "cam0=[88.5 0.02 46.25; 0 87.75 31.0; 0 0 1]\ndist0=[0.01 -0.003 0.0005 -0.0004 0.001]\n"
      "cam1=[90.0 -0.01 48.5; 0 91.5 32.25; 0 0 1]\ndist1=[-0.008 0.002 -0.0003 0.0006 0]\n"
      "R=[0.9998 0.0076 -0.0185; -0.0078 0.9999 -0.0108; 0.0184 0.0109 0.9998]\nT=[-0.2 0.01 -0.015]\nwidth=96\nheight=64\nextra=ignored\n";
  cspm_rig rig;
  EXPECT(ParseRig(text, std::strlen(text), &rig));
  EXPECT(rig.raw_w == 96 && rig.raw_h == 64 && rig.cam[0].skew == 0.02 && rig.cam[1].fy == 91.5 && rig.cam[0].k3 == 0.001 && rig.cam[1].p2 == 0.0006);
  EXPECT(rig.R[5] == -0.0108 && rig.T[0] == -0.2);
  cspm_rig junk;
  EXPECT(!ParseRig(text, std::strlen(text) - 30, &junk));  // cut inside width=: a key is missing
  EXPECT(!ParseRig("", 0, &junk));
  const std::string twice = std::string(text) + "T=[-0.3 0 0]\n";  // a repeated key is a mistake, not an override
  EXPECT(!ParseRig(twice.data(), twice.size(), &junk));
  cspm_rect_params rp;
  cspm_rect_default_params(&rp);
  rp.w = 90;
  rp.h = 50;
  cspm_rectification rect;
  cspm_calib calib;
  EXPECT(cspm_rectify_compute(&rig, &rp, &rect, &calib) == CSPM_OK);
  EXPECT(rect.w == 90 && rect.h == 50 && calib.doffs == 0.0 && calib.baseline == rect.baseline);
  const int max_dis = 16;
  try {
    const Mat l_raw = Noise(96, 64, 1u), r_raw = Noise(96, 64, 2u), l2 = Noise(96, 64, 3u), r2 = Noise(96, 64, 4u);
    Mat l_rect, r_rect, l_valid, r_valid;
    RectifyPair(rig, rect, l_raw, r_raw, l_rect, r_rect, &l_valid, &r_valid);
    EXPECT(l_rect.cols == 90 && l_rect.rows == 50 && l_rect.type() == CV_8UC3 && l_valid.type() == CV_8UC1);
    for (int v = 0; v < 2; ++v) {  // == the C ABI
      Mat want(50, 90, CV_8UC3), mask(50, 90, CV_8UC1);
      const Mat &raw = v ? r_raw : l_raw;
      EXPECT(cspm_rectify_host(0, &rig, &rect, v, raw.data, raw.step, want.data, want.step, NULL, mask.data) == CSPM_OK);
      EXPECT(SameMat(want, v ? r_rect : l_rect) && SameMat(mask, v ? r_valid : l_valid));
      size_t valid = 0;
      for (int y = 0; y < 50; ++y)
        for (int x = 0; x < 90; ++x) valid += mask.ptr<unsigned char>(y)[x] != 0;
      EXPECT(valid > 1000 && valid <= 4500);
    }
    GrdCC cc;
    Mat dis_slot[2], dis_plain[2];
    {
      DeviceSlot slot(0, /*keep_context=*/true);
      DeviceSlot::Use use(slot);
      slot.SetRectification(&rig, &rect);
      EXPECT(slot.rectifies());
      {
        PreSSPC pc(l_raw, r_raw, max_dis, 9, &cc);
        Mat a, b;
        pc.LevelImages(&a, &b);
        EXPECT(SameMat(a, l_rect) && SameMat(b, r_rect));
      }
      {  // the parked context: its maps serve the next raw pair
        PreSSPC pc(l2, r2, max_dis, 9, &cc);
        Mat a, b, a2, b2;
        pc.LevelImages(&a, &b);
        RectifyPair(rig, rect, l2, r2, a2, b2, NULL, NULL);
        EXPECT(SameMat(a, a2) && SameMat(b, b2));
        CSPatchMatch m(l2, r2, rig, rect, max_dis, 4);
        m.set_seed(5);
        m.PatchMatch(1, &pc, false);
        dis_slot[0] = m.dis(kLeft).clone();
        dis_slot[1] = m.dis(kRight).clone();
      }
      bool threw = false;
      try {
        PreSSPC pc(Noise(80, 64, 5u), Noise(80, 64, 6u), max_dis, 9, &cc);
      } catch (const std::exception &) {
        threw = true;
      }
      EXPECT(threw);
      slot.SetRectification(NULL, NULL);
      EXPECT(!slot.rectifies());
      {  // the same slot without a rectification: the ordinary flow on the rectified pair gives the same maps
        Mat a2, b2;
        RectifyPair(rig, rect, l2, r2, a2, b2, NULL, NULL);
        PreSSPC pc(a2, b2, max_dis, 9, &cc);
        CSPatchMatch m(a2, b2, max_dis, 4);
        m.set_seed(5);
        m.PatchMatch(1, &pc, false);
        dis_plain[0] = m.dis(kLeft).clone();
        dis_plain[1] = m.dis(kRight).clone();
      }
    }
    EXPECT(dis_slot[0].cols == 90 && dis_slot[0].rows == 50);
    EXPECT(SameMat(dis_slot[0], dis_plain[0]) && SameMat(dis_slot[1], dis_plain[1]));
    bool threw = false;
    try {
      Mat a, b;
      RectifyPair(rig, rect, Noise(80, 64, 7u), r_raw, a, b, NULL, NULL);
    } catch (const std::exception &) {
      threw = true;
    }
    EXPECT(threw);
  } catch (const std::exception &e) {
    std::printf("FAILED: %s\n", e.what());
    ++g_bad;
  }
  if (g_bad) return 1;
  std::printf("rect_check ok\n");
  return 0;
}
