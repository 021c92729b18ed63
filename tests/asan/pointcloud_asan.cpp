// Host-side AddressSanitizer run of the point cloud's two entries
// (lea_disparity_pointcloud_workspace_bytes, lea_disparity_pointcloud_f32), built and run by
// `make asan` after the other drivers, the same way: every csrc unit with ASan on its host
// side, nothing launched.  Each refused call must return LEA_E_INVALID, leave a
// lea_last_error() that names the entry, and touch none of its buffers.
// Exit 0 = every check passed and ASan saw no error.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "leastereo_hip.h"

static int g_fail = 0;

static void expect_err(const char* entry, const char* what, int rc, int want) {
  const char* e = lea_last_error();
  if (rc != want || e == nullptr || std::strstr(e, entry) == nullptr) {
    std::printf("FAIL %s %s: rc=%d (want %d) err='%s'\n", entry, what, rc, want, e ? e : "(null)");
    ++g_fail;
  }
}

static void expect_bytes(const char* what, size_t got, size_t want) {
  if (got != want) {
    std::printf("FAIL workspace bytes %s: %zu (want %zu)\n", what, got, want);
    ++g_fail;
  }
}

// B = 2, H = 6, W = 7: a map is 84 pixels, the workspace one int per image; capacity 10
constexpr int kMap = 84, kCap = 10, kRows = 2 * kCap;
static float disp[kMap], pts[3 * kMap], xyz[3 * kRows], nrm[3 * kRows], Q[32];
static int32_t ws[8], cnt[2], idx[kRows];
static uint8_t ex[kMap], img[4 * kMap], val[kMap], rgb[3 * kRows];

struct Args {
  const float* d = disp;
  const uint8_t* e = ex;
  const void* im = img;
  int ps = 3;
  const float* q = Q;
  int64_t qs = 16;
  int B = 2, H = 6, W = 7;
  float lo = 0.f, hi = 192.f, nmd = 1.f;
  int cap = kCap;
  void* w = ws;
  float* points = pts;
  uint8_t* valid = val;
  int32_t* count = cnt;
  float* x = xyz;
  uint8_t* c = rgb;
  int32_t* i = idx;
  float* n = nrm;
};

static int call(const Args& a) {
  return lea_disparity_pointcloud_f32(a.d, a.e, a.im, a.ps, a.q, a.qs, a.B, a.H, a.W, a.lo, a.hi, a.nmd, a.cap, a.w,
                                      a.points, a.valid, a.count, a.x, a.c, a.i, a.n, nullptr);
}

template <class F>
static void refused(const char* what, F change) {
  Args a;
  change(a);
  expect_err("lea_disparity_pointcloud_f32", what, call(a), LEA_E_INVALID);
}

int main() {
  if (lea_abi_version() != 14) {
    std::printf("FAIL abi version %d\n", lea_abi_version());
    ++g_fail;
  }
  // one int per block of 1024 pixels per image
  expect_bytes("2x6x7", lea_disparity_pointcloud_workspace_bytes(2, 6, 7), 8);
  expect_bytes("1x1x1", lea_disparity_pointcloud_workspace_bytes(1, 1, 1), 4);
  expect_bytes("1x32x32", lea_disparity_pointcloud_workspace_bytes(1, 32, 32), 4);
  expect_bytes("1x1x1025", lea_disparity_pointcloud_workspace_bytes(1, 1, 1025), 8);
  expect_bytes("3x2048x2048", lea_disparity_pointcloud_workspace_bytes(3, 2048, 2048), (size_t)3 * 4096 * 4);
  expect_bytes("3x40000x50000", lea_disparity_pointcloud_workspace_bytes(3, 40000, 50000), (size_t)3 * 1953125 * 4);
  expect_bytes("B = 0", lea_disparity_pointcloud_workspace_bytes(0, 6, 7), 0);
  expect_bytes("H < 0", lea_disparity_pointcloud_workspace_bytes(2, -6, 7), 0);
  expect_bytes("W = 0", lea_disparity_pointcloud_workspace_bytes(2, 6, 0), 0);

  auto reset = [&]() {
    for (float& v : disp) v = -7.f;
    for (float& v : pts) v = -7.f;
    for (float& v : xyz) v = -7.f;
    for (float& v : nrm) v = -7.f;
    for (float& v : Q) v = -7.f;
    for (int32_t& v : ws) v = -7;
    for (int32_t& v : cnt) v = -7;
    for (int32_t& v : idx) v = -7;
    for (uint8_t& v : ex) v = 9;
    for (uint8_t& v : img) v = 9;
    for (uint8_t& v : val) v = 9;
    for (uint8_t& v : rgb) v = 9;
  };
  reset();
  const float nan = std::nanf("");

  refused("null disp", [](Args& a) { a.d = nullptr; });
  refused("null Q", [](Args& a) { a.q = nullptr; });
  refused("null workspace", [](Args& a) { a.w = nullptr; });
  refused("every output null", [](Args& a) {
    a.points = nullptr, a.valid = nullptr, a.count = nullptr, a.x = nullptr, a.c = nullptr, a.i = nullptr,
    a.n = nullptr;
  });
  refused("rgb without image", [](Args& a) { a.im = nullptr; });
  refused("pix_stride 2", [](Args& a) { a.ps = 2; });
  refused("pix_stride 5", [](Args& a) { a.ps = 5; });
  refused("pix_stride 0", [](Args& a) { a.ps = 0; });
  refused("B = 0", [](Args& a) { a.B = 0; });
  refused("B < 0", [](Args& a) { a.B = -2; });
  refused("H < 0", [](Args& a) { a.H = -6; });
  refused("W = 0", [](Args& a) { a.W = 0; });
  refused("B too large", [](Args& a) { a.B = 65536, a.H = 1, a.W = 1; });
  refused("H*W = 2^31", [](Args& a) { a.B = 1, a.H = 1 << 16, a.W = 1 << 15; });
  refused("H*W = 2^40", [](Args& a) { a.B = 1, a.H = 1 << 20, a.W = 1 << 20; });
  refused("B*H*W = 2^31", [](Args& a) { a.B = 2, a.H = 1 << 15, a.W = 1 << 15; });
  refused("Q stride 8", [](Args& a) { a.qs = 8; });
  refused("Q stride < 0", [](Args& a) { a.qs = -16; });
  refused("capacity < 0", [](Args& a) { a.cap = -1; });
  refused("capacity 0 with xyz", [](Args& a) { a.cap = 0; });
  refused("capacity 0 with index alone", [](Args& a) {
    a.cap = 0, a.points = nullptr, a.valid = nullptr, a.count = nullptr, a.x = nullptr, a.c = nullptr, a.n = nullptr;
  });
  refused("min_disp NaN", [nan](Args& a) { a.lo = nan; });
  refused("max_disp NaN", [nan](Args& a) { a.hi = nan; });
  refused("normal_max_diff NaN", [nan](Args& a) { a.nmd = nan; });
  refused("normal_max_diff < 0", [](Args& a) { a.nmd = -0.5f; });
  refused("misaligned workspace", [](Args& a) { a.w = (char*)ws + 2; });
  // an output on an input
  refused("points = disp", [](Args& a) { a.points = disp; });
  refused("xyz = disp", [](Args& a) { a.x = disp; });
  refused("valid = exclude", [](Args& a) { a.valid = ex; });
  refused("valid starts in exclude's last byte", [](Args& a) { a.valid = ex + kMap - 1; });
  refused("rgb = image", [](Args& a) { a.c = img; });
  refused("rgb in the image's last byte (stride 4)", [](Args& a) { a.ps = 4, a.c = img + 4 * kMap - 1; });
  refused("count = Q", [](Args& a) { a.count = (int32_t*)Q; });
  refused("index in the second matrix", [](Args& a) { a.i = (int32_t*)(Q + 31); });
  refused("normals in the workspace", [](Args& a) { a.n = (float*)ws; });
  refused("count in the workspace's last int", [](Args& a) { a.count = ws + 1; });
  // an output on another output
  refused("xyz = normals", [](Args& a) { a.x = nrm; });
  refused("valid in points' last byte", [](Args& a) { a.valid = (uint8_t*)pts + 12 * kMap - 1; });
  refused("index = count", [](Args& a) { a.i = cnt; });
  refused("rgb in xyz's last byte", [](Args& a) { a.c = (uint8_t*)xyz + 12 * kRows - 1; });
  refused("normals = points", [](Args& a) { a.n = pts; });
  // the workspace on an input
  refused("workspace = disp", [](Args& a) { a.w = disp; });
  refused("workspace = Q", [](Args& a) { a.w = Q; });
  refused("workspace ends in exclude", [](Args& a) { a.w = (void*)(((uintptr_t)ex & ~(uintptr_t)3) - 4); });
  // the optional ones may be null: the next check in line fires
  refused("null exclude, image and all but count, then capacity", [](Args& a) {
    a.e = nullptr, a.im = nullptr, a.ps = 0, a.points = nullptr, a.valid = nullptr, a.x = nullptr, a.c = nullptr,
    a.i = nullptr, a.n = nullptr, a.cap = -3;
  });
  // with one matrix for all (stride 0) only its 16 floats are Q: an output behind them is
  // no overlap, and the next check in line fires
  refused("Q stride 0, count behind the matrix, then the workspace", [](Args& a) {
    a.qs = 0, a.count = (int32_t*)(Q + 16), a.w = (char*)ws + 1;
  });

  bool wrote = false;
  for (float v : disp) wrote |= v != -7.f;
  for (float v : pts) wrote |= v != -7.f;
  for (float v : xyz) wrote |= v != -7.f;
  for (float v : nrm) wrote |= v != -7.f;
  for (float v : Q) wrote |= v != -7.f;
  for (int32_t v : ws) wrote |= v != -7;
  for (int32_t v : cnt) wrote |= v != -7;
  for (int32_t v : idx) wrote |= v != -7;
  for (uint8_t v : ex) wrote |= v != 9;
  for (uint8_t v : img) wrote |= v != 9;
  for (uint8_t v : val) wrote |= v != 9;
  for (uint8_t v : rgb) wrote |= v != 9;
  if (wrote) {
    std::printf("FAIL a refused call wrote to a buffer\n");
    ++g_fail;
  }
  if (g_fail)
    std::printf("FAIL pointcloud: %d failed checks\n", g_fail);
  else
    std::printf("OK: 0 failed checks\n");
  return g_fail ? 1 : 0;
}
