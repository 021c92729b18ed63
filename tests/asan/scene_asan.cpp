// Host-side AddressSanitizer run of whole-scene inference's entries
// (lea_standardize_tiles_workspace_bytes, lea_standardize_tiles_u8, lea_tile_blend_f32), built
// and run by `make asan` after the other drivers, the same way: every csrc unit with ASan on
// its host side, nothing launched.  Each refused call must return LEA_E_INVALID, leave a
// lea_last_error() that names the entry, and touch none of its buffers.
// Exit 0 = every check passed and ASan saw no error.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "leastereo_hip.h"

static int g_fail = 0;

static void expect_err(const char* entry, const char* what, int rc, int want) {
  const char* e = lea_last_error();
  if (rc != want || e == nullptr || std::strstr(e, entry) == nullptr) {
    std::printf("FAIL %s %s: rc=%d (want %d) err='%s'\n", entry, what, rc, want, e ? e : "(null)");
    ++g_fail;
  }
}

int main() {
  if (lea_abi_version() != 14) {
    std::printf("FAIL abi version %d\n", lea_abi_version());
    ++g_fail;
  }
  if (lea_standardize_tiles_workspace_bytes() != 2 * 3 * 2 * sizeof(unsigned long long) ||
      lea_standardize_tiles_workspace_bytes() != lea_standardize_workspace_bytes(1)) {
    std::printf("FAIL lea_standardize_tiles_workspace_bytes\n");
    ++g_fail;
  }
  // a 6 x 7 RGB scene, N = 2 tiles of 4 x 8; host memory, the checks never dereference it
  constexpr int kPix = 6 * 7, kTile = 4 * 8;
  alignas(16) static unsigned char img[2][kPix * 3];
  alignas(16) static float out[2][2 * 3 * kTile];
  alignas(16) static int origins[2 * 2 + 2];
  alignas(16) static unsigned long long ws[2 * 3 * 2];
  std::memset(img, 0x5a, sizeof img);
  for (auto& o : out)
    for (float& v : o) v = -7.f;
  for (int& v : origins) v = -7;
  for (auto& v : ws) v = 7;
  {
    const char* who = "lea_standardize_tiles_u8";
    auto call = [&](const void* l, const void* r, int H, int W, int ps, const int* o, int N, float* ol, float* orr,
                    int th, int tw, void* w) {
      return lea_standardize_tiles_u8(l, r, H, W, ps, o, N, ol, orr, th, tw, w, nullptr);
    };
    const void *L = img[0], *R = img[1];
    float *OL = out[0], *OR = out[1];
    expect_err(who, "null left", call(nullptr, R, 6, 7, 3, origins, 2, OL, OR, 4, 8, ws), LEA_E_INVALID);
    expect_err(who, "null right", call(L, nullptr, 6, 7, 3, origins, 2, OL, OR, 4, 8, ws), LEA_E_INVALID);
    expect_err(who, "null origins", call(L, R, 6, 7, 3, nullptr, 2, OL, OR, 4, 8, ws), LEA_E_INVALID);
    expect_err(who, "null out_left", call(L, R, 6, 7, 3, origins, 2, nullptr, OR, 4, 8, ws), LEA_E_INVALID);
    expect_err(who, "null out_right", call(L, R, 6, 7, 3, origins, 2, OL, nullptr, 4, 8, ws), LEA_E_INVALID);
    expect_err(who, "null workspace", call(L, R, 6, 7, 3, origins, 2, OL, OR, 4, 8, nullptr), LEA_E_INVALID);
    expect_err(who, "N = 0", call(L, R, 6, 7, 3, origins, 0, OL, OR, 4, 8, ws), LEA_E_INVALID);
    expect_err(who, "N < 0", call(L, R, 6, 7, 3, origins, -2, OL, OR, 4, 8, ws), LEA_E_INVALID);
    expect_err(who, "N = 65536", call(L, R, 6, 7, 3, origins, 65536, OL, OR, 4, 8, ws), LEA_E_INVALID);
    expect_err(who, "H = 0", call(L, R, 0, 7, 3, origins, 2, OL, OR, 4, 8, ws), LEA_E_INVALID);
    expect_err(who, "W < 0", call(L, R, 6, -7, 3, origins, 2, OL, OR, 4, 8, ws), LEA_E_INVALID);
    expect_err(who, "tile_h = 0", call(L, R, 6, 7, 3, origins, 2, OL, OR, 0, 8, ws), LEA_E_INVALID);
    expect_err(who, "tile_w < 0", call(L, R, 6, 7, 3, origins, 2, OL, OR, 4, -8, ws), LEA_E_INVALID);
    expect_err(who, "pix_stride 2", call(L, R, 6, 7, 2, origins, 2, OL, OR, 4, 8, ws), LEA_E_INVALID);
    expect_err(who, "pix_stride 5", call(L, R, 6, 7, 5, origins, 2, OL, OR, 4, 8, ws), LEA_E_INVALID);
    expect_err(who, "scene of 2^31 pixels", call(L, R, 1 << 16, 1 << 15, 3, origins, 2, OL, OR, 4, 8, ws),
               LEA_E_INVALID);
    expect_err(who, "tile of 2^31 pixels", call(L, R, 6, 7, 3, origins, 2, OL, OR, 1 << 16, 1 << 15, ws),
               LEA_E_INVALID);
    expect_err(who, "misaligned out, tile_w % 4 == 0", call(L, R, 6, 7, 3, origins, 2, OL, OR + 1, 4, 8, ws),
               LEA_E_INVALID);
    expect_err(who, "misaligned origins",
               call(L, R, 6, 7, 3, (const int*)((const char*)origins + 2), 2, OL, OR, 4, 8, ws), LEA_E_INVALID);
    expect_err(who, "misaligned workspace", call(L, R, 6, 7, 3, origins, 2, OL, OR, 4, 8, (char*)ws + 4),
               LEA_E_INVALID);
  }
  // 2 x 1 tiles of 4 x 8 blended into 6 x 8
  alignas(16) static float tiles[2 * kTile];
  alignas(16) static float scene[6 * 8];
  for (float& v : tiles) v = -7.f;
  for (float& v : scene) v = -7.f;
  int* ys = origins;
  int* xs = origins + 2;
  int* cnt = origins + 4;
  {
    const char* who = "lea_tile_blend_f32";
    auto call = [&](const float* t, int64_t bs, const int* y, int ny, const int* x, int nx, int th, int tw, int gy0,
                    int gy1, int gx0, int gx1, int ramp, float* o, int H, int W, int* c) {
      return lea_tile_blend_f32(t, bs, y, ny, x, nx, th, tw, gy0, gy1, gx0, gx1, ramp, o, H, W, c, nullptr);
    };
    expect_err(who, "null tiles", call(nullptr, kTile, ys, 2, xs, 1, 4, 8, 1, 1, 2, 1, 1, scene, 6, 8, cnt),
               LEA_E_INVALID);
    expect_err(who, "null ys", call(tiles, kTile, nullptr, 2, xs, 1, 4, 8, 1, 1, 2, 1, 1, scene, 6, 8, cnt),
               LEA_E_INVALID);
    expect_err(who, "null xs", call(tiles, kTile, ys, 2, nullptr, 1, 4, 8, 1, 1, 2, 1, 1, scene, 6, 8, cnt),
               LEA_E_INVALID);
    expect_err(who, "null out", call(tiles, kTile, ys, 2, xs, 1, 4, 8, 1, 1, 2, 1, 1, nullptr, 6, 8, cnt),
               LEA_E_INVALID);
    expect_err(who, "ny = 0", call(tiles, kTile, ys, 0, xs, 1, 4, 8, 1, 1, 2, 1, 1, scene, 6, 8, cnt), LEA_E_INVALID);
    expect_err(who, "nx < 0", call(tiles, kTile, ys, 2, xs, -1, 4, 8, 1, 1, 2, 1, 1, scene, 6, 8, cnt), LEA_E_INVALID);
    expect_err(who, "ny = 65", call(tiles, kTile, ys, 65, xs, 1, 4, 8, 1, 1, 2, 1, 1, scene, 6, 8, cnt), LEA_E_INVALID);
    expect_err(who, "nx = 65", call(tiles, kTile, ys, 2, xs, 65, 4, 8, 1, 1, 2, 1, 1, scene, 6, 8, cnt), LEA_E_INVALID);
    expect_err(who, "tile_h = 0", call(tiles, kTile, ys, 2, xs, 1, 0, 8, 1, 1, 2, 1, 1, scene, 6, 8, cnt),
               LEA_E_INVALID);
    expect_err(who, "tile_w < 0", call(tiles, kTile, ys, 2, xs, 1, 4, -8, 1, 1, 2, 1, 1, scene, 6, 8, cnt),
               LEA_E_INVALID);
    expect_err(who, "H = 0", call(tiles, kTile, ys, 2, xs, 1, 4, 8, 1, 1, 2, 1, 1, scene, 0, 8, cnt), LEA_E_INVALID);
    expect_err(who, "W < 0", call(tiles, kTile, ys, 2, xs, 1, 4, 8, 1, 1, 2, 1, 1, scene, 6, -8, cnt), LEA_E_INVALID);
    expect_err(who, "scene of 2^31 pixels",
               call(tiles, kTile, ys, 2, xs, 1, 4, 8, 1, 1, 2, 1, 1, scene, 1 << 16, 1 << 15, cnt), LEA_E_INVALID);
    expect_err(who, "tile of 2^31 pixels",
               call(tiles, (int64_t)1 << 31, ys, 2, xs, 1, 1 << 16, 1 << 15, 1, 1, 2, 1, 1, scene, 6, 8, cnt),
               LEA_E_INVALID);
    expect_err(who, "batch stride below the tile", call(tiles, kTile - 1, ys, 2, xs, 1, 4, 8, 1, 1, 2, 1, 1, scene, 6, 8, cnt),
               LEA_E_INVALID);
    expect_err(who, "negative batch stride", call(tiles, -kTile, ys, 2, xs, 1, 4, 8, 1, 1, 2, 1, 1, scene, 6, 8, cnt),
               LEA_E_INVALID);
    expect_err(who, "ramp 0", call(tiles, kTile, ys, 2, xs, 1, 4, 8, 1, 1, 2, 1, 0, scene, 6, 8, cnt), LEA_E_INVALID);
    expect_err(who, "ramp 257", call(tiles, kTile, ys, 2, xs, 1, 4, 8, 1, 1, 2, 1, 257, scene, 6, 8, cnt),
               LEA_E_INVALID);
    expect_err(who, "guard_y0 < 0", call(tiles, kTile, ys, 2, xs, 1, 4, 8, -1, 1, 2, 1, 1, scene, 6, 8, cnt),
               LEA_E_INVALID);
    expect_err(who, "guard_y1 < 0", call(tiles, kTile, ys, 2, xs, 1, 4, 8, 1, -1, 2, 1, 1, scene, 6, 8, cnt),
               LEA_E_INVALID);
    expect_err(who, "guard_x0 < 0", call(tiles, kTile, ys, 2, xs, 1, 4, 8, 1, 1, -2, 1, 1, scene, 6, 8, cnt),
               LEA_E_INVALID);
    expect_err(who, "guard_x1 < 0", call(tiles, kTile, ys, 2, xs, 1, 4, 8, 1, 1, 2, -1, 1, scene, 6, 8, cnt),
               LEA_E_INVALID);
    expect_err(who, "out aliases tiles", call(tiles, kTile, ys, 2, xs, 1, 4, 8, 1, 1, 2, 1, 1, tiles, 6, 8, cnt),
               LEA_E_INVALID);
    expect_err(who, "misaligned out, W % 4 == 0",
               call(tiles, kTile, ys, 2, xs, 1, 4, 8, 1, 1, 2, 1, 1, scene + 1, 6, 8, cnt), LEA_E_INVALID);
    expect_err(who, "misaligned ys",
               call(tiles, kTile, (const int*)((const char*)ys + 2), 2, xs, 1, 4, 8, 1, 1, 2, 1, 1, scene, 6, 8, cnt),
               LEA_E_INVALID);
    // the optional count is not what a refusal is about: still the shape
    expect_err(who, "ny = 0 without a count", call(tiles, kTile, ys, 0, xs, 1, 4, 8, 1, 1, 2, 1, 1, scene, 6, 8, nullptr),
               LEA_E_INVALID);
  }
  bool wrote = false;
  for (auto& o : out)
    for (float v : o) wrote = wrote || v != -7.f;
  for (float v : tiles) wrote = wrote || v != -7.f;
  for (float v : scene) wrote = wrote || v != -7.f;
  if (wrote) {
    std::printf("FAIL a refused call wrote to an output or to the tiles\n");
    ++g_fail;
  }
  for (int v : origins)
    if (v != -7) {
      std::printf("FAIL a refused call wrote to the origins or the count\n");
      ++g_fail;
      break;
    }
  for (auto v : ws)
    if (v != 7) {
      std::printf("FAIL a refused call wrote to the workspace\n");
      ++g_fail;
      break;
    }
  std::printf("%s scene: %d failed checks\n", g_fail ? "FAIL" : "OK", g_fail);
  return g_fail ? 1 : 0;
}
