// ply_io.h -- a point cloud of cspm_point records (include/cspm.h "reprojection") as a binary little-endian PLY: per vertex
// x y z nx ny nz as float and red green blue as uchar, 27 bytes.  A normal with a NaN component is written as 0 0 0 (viewers take a zero
// normal for "none"; a NaN makes several of them drop the file).
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/cspm.h"

static_assert(sizeof(cspm_point) == 32, "cspm_point is one 32-byte record");

inline bool WritePLY(const std::string &path, const cspm_point *pts, size_t n) {
  FILE *fp = std::fopen(path.c_str(), "wb");
  if (!fp) return false;
  std::fprintf(fp,
               "ply\nformat binary_little_endian 1.0\nelement vertex %zu\nproperty float x\nproperty float y\nproperty float z\n"
               "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n",
               n);
  const uint16_t one = 1;
  const bool host_little = *reinterpret_cast<const unsigned char *>(&one) == 1;
  constexpr size_t kRec = 27, kChunk = 4096;
  std::vector<unsigned char> buf(kRec * kChunk);
  bool ok = true;
  for (size_t i0 = 0; i0 < n && ok; i0 += kChunk) {
    const size_t m = n - i0 < kChunk ? n - i0 : kChunk;
    for (size_t j = 0; j < m; ++j) {
      const cspm_point &p = pts[i0 + j];
      float v[6] = {p.x, p.y, p.z, p.nx, p.ny, p.nz};
      if (v[3] != v[3] || v[4] != v[4] || v[5] != v[5]) v[3] = v[4] = v[5] = 0.0f;
      unsigned char *o = buf.data() + kRec * j;
      for (int k = 0; k < 6; ++k) {
        unsigned char b[4];
        std::memcpy(b, &v[k], 4);
        if (!host_little) { const unsigned char t0 = b[0], t1 = b[1]; b[0] = b[3]; b[1] = b[2]; b[2] = t1; b[3] = t0; }
        std::memcpy(o + 4 * k, b, 4);
      }
      o[24] = p.r; o[25] = p.g; o[26] = p.b;
    }
    ok = std::fwrite(buf.data(), kRec, m, fp) == m;
  }
  return std::fclose(fp) == 0 && ok;
}

// A triangle mesh (include/cspm.h "triangle meshes"): the vertex block of WritePLY, byte for byte, then one 13-byte record per face: the
// count 3 as uchar and the three vertex numbers as little-endian int32 ("property list uchar int vertex_indices").
static_assert(sizeof(cspm_face) == 12, "cspm_face is one 12-byte record");

inline bool WritePLYMesh(const std::string &path, const cspm_point *pts, size_t nv, const cspm_face *faces, size_t nf) {
  FILE *fp = std::fopen(path.c_str(), "wb");
  if (!fp) return false;
  std::fprintf(fp,
               "ply\nformat binary_little_endian 1.0\nelement vertex %zu\nproperty float x\nproperty float y\nproperty float z\n"
               "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
               "element face %zu\nproperty list uchar int vertex_indices\nend_header\n",
               nv, nf);
  const uint16_t one = 1;
  const bool host_little = *reinterpret_cast<const unsigned char *>(&one) == 1;
  constexpr size_t kRec = 27, kFace = 13, kChunk = 4096;
  std::vector<unsigned char> buf(kRec * kChunk);
  bool ok = true;
  for (size_t i0 = 0; i0 < nv && ok; i0 += kChunk) {
    const size_t m = nv - i0 < kChunk ? nv - i0 : kChunk;
    for (size_t j = 0; j < m; ++j) {
      const cspm_point &p = pts[i0 + j];
      float v[6] = {p.x, p.y, p.z, p.nx, p.ny, p.nz};
      if (v[3] != v[3] || v[4] != v[4] || v[5] != v[5]) v[3] = v[4] = v[5] = 0.0f;
      unsigned char *o = buf.data() + kRec * j;
      for (int k = 0; k < 6; ++k) {
        unsigned char b[4];
        std::memcpy(b, &v[k], 4);
        if (!host_little) { const unsigned char t0 = b[0], t1 = b[1]; b[0] = b[3]; b[1] = b[2]; b[2] = t1; b[3] = t0; }
        std::memcpy(o + 4 * k, b, 4);
      }
      o[24] = p.r; o[25] = p.g; o[26] = p.b;
    }
    ok = std::fwrite(buf.data(), kRec, m, fp) == m;
  }
  for (size_t i0 = 0; i0 < nf && ok; i0 += kChunk) {
    const size_t m = nf - i0 < kChunk ? nf - i0 : kChunk;
    for (size_t j = 0; j < m; ++j) {
      unsigned char *o = buf.data() + kFace * j;
      o[0] = 3;
      for (int k = 0; k < 3; ++k) {
        const uint32_t v = faces[i0 + j].v[k];
        o[1 + 4 * k] = (unsigned char)(v & 255u);
        o[2 + 4 * k] = (unsigned char)(v >> 8 & 255u);
        o[3 + 4 * k] = (unsigned char)(v >> 16 & 255u);
        o[4 + 4 * k] = (unsigned char)(v >> 24 & 255u);
      }
    }
    ok = std::fwrite(buf.data(), kFace, m, fp) == m;
  }
  return std::fclose(fp) == 0 && ok;
}
