// pfm_io.h -- float disparity maps as single-channel PFM ("Pf", little-endian, rows bottom-up), the format the
// Middlebury / KITTI tooling reads.  The reference writes only 8-bit maps quantised by dis_scale
// (CSPM/main.cc:133-134, cs_patchmatch.cc:590-601); the float file keeps the sub-pixel plane disparities.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

inline bool WritePFM(const std::string &path, const double *disp, int w, int h) {
  FILE *fp = std::fopen(path.c_str(), "wb");
  if (!fp) return false;
  std::fprintf(fp, "Pf\n%d %d\n-1.0\n", w, h);  // negative scale = little-endian
  std::vector<float> row((size_t)w);
  bool ok = true;
  for (int y = h - 1; y >= 0 && ok; --y) {
    for (int x = 0; x < w; ++x) row[x] = (float)disp[(size_t)y * w + x];
    ok = std::fwrite(row.data(), sizeof(float), (size_t)w, fp) == (size_t)w;
  }
  return std::fclose(fp) == 0 && ok;
}

// a single-channel PFM ("Pf") of either byte order into row-major doubles, top row first; false for anything else
inline bool ReadPFM(const std::string &path, std::vector<double> *disp, int *w, int *h) {
  FILE *fp = std::fopen(path.c_str(), "rb");
  if (!fp) return false;
  char tag[3] = {0, 0, 0};
  double scale = 0.0;
  bool ok = std::fscanf(fp, "%2s %d %d %lf", tag, w, h, &scale) == 4 && tag[0] == 'P' && tag[1] == 'f' && *w > 0 && *h > 0 && scale != 0.0;
  ok = ok && std::fgetc(fp) != EOF;  // the single whitespace byte after the header
  if (ok) {
    const uint16_t one = 1;
    const bool host_little = *reinterpret_cast<const unsigned char *>(&one) == 1;
    const bool swap = (scale < 0.0) != host_little;
    std::vector<float> row((size_t)*w);
    disp->resize((size_t)*w * *h);
    for (int y = *h - 1; y >= 0 && ok; --y) {
      ok = std::fread(row.data(), sizeof(float), (size_t)*w, fp) == (size_t)*w;
      for (int x = 0; x < *w && ok; ++x) {
        if (swap) {
          unsigned char *b = reinterpret_cast<unsigned char *>(&row[x]);
          const unsigned char t0 = b[0], t1 = b[1];
          b[0] = b[3]; b[1] = b[2]; b[2] = t1; b[3] = t0;
        }
        (*disp)[(size_t)y * *w + x] = (double)row[x];
      }
    }
  }
  std::fclose(fp);
  return ok;
}
