// mesh_io_check.cc -- the host layer's mesh writer (host/ply_io.h WritePLYMesh), stand-alone: no device, no library.  Writes the small
// mesh that tests/test_mesh_ref.py reads back byte for byte, one more with more faces than a write chunk holds, and an empty one.
// usage: mesh_io_check OUT.ply        prints "mesh_io_check ok" and exits 0, or says what failed and exits 1
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "ply_io.h"

static int g_bad = 0;
#define EXPECT(cond)                                        \
  do {                                                      \
    if (!(cond)) {                                          \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
      ++g_bad;                                              \
    }                                                       \
  } while (0)

static long FileSize(const std::string &path) {
  FILE *fp = std::fopen(path.c_str(), "rb");
  if (!fp) return -1;
  std::fseek(fp, 0, SEEK_END);
  const long n = std::ftell(fp);
  std::fclose(fp);
  return n;
}

int main(int argc, char **argv) {
  if (argc != 2) {
    std::printf("usage: mesh_io_check OUT.ply\n");
    return 2;
  }
  const std::string out = argv[1];
  const float nan = std::numeric_limits<float>::quiet_NaN();
  const cspm_point pts[4] = {{1.f, 2.f, 3.f, 0.f, 0.f, -1.f, 10, 20, 30, 255, 0u},
                             {-0.5f, 0.25f, 8.f, 0.6f, 0.f, -0.8f, 255, 0, 128, 255, 1u},
                             {4.f, 5.f, 6.f, nan, 0.5f, 0.5f, 9, 8, 7, 255, 5u},
                             {7.f, 8.f, 9.f, 0.f, 1.f, 0.f, 1, 2, 3, 255, 6u}};
  const cspm_face faces[2] = {{{0u, 2u, 3u}}, {{0u, 3u, 0x01020304u}}};
  EXPECT(WritePLYMesh(out, pts, 4, faces, 2));
  EXPECT(!WritePLYMesh(out + ".no-such-dir/x.ply", pts, 4, faces, 2));
  // the vertex block is WritePLY's, byte for byte: the mesh file is the cloud file with another header and the faces behind it
  EXPECT(WritePLY(out + ".cloud", pts, 4));
  // more records than one write chunk, exact buffers: a read or write past an end is a sanitizer finding
  const size_t nv = 4096 + 3, nf = 2 * 4096 + 1;
  std::vector<cspm_point> many(nv, pts[1]);
  std::vector<cspm_face> tri(nf, faces[0]);
  EXPECT(WritePLYMesh(out + ".big", many.data(), nv, tri.data(), nf));
  const long big = FileSize(out + ".big");
  EXPECT(big > 0 && (size_t)big > 27 * nv + 13 * nf && (size_t)big < 27 * nv + 13 * nf + 512);
  EXPECT(WritePLYMesh(out + ".empty", nullptr, 0, nullptr, 0));
  EXPECT(FileSize(out + ".empty") > 0 && FileSize(out + ".empty") < 512);
  if (g_bad) return 1;
  std::printf("mesh_io_check ok\n");
  return 0;
}
